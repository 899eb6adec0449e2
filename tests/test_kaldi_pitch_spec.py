"""Kaldi's pitch features without a GPU: the lag grid and the frame count of kaldi_pitch.KaldiPitch, its float32 twin against
its float64 specification within the bounds the module derives, the decode against a brute-force Viterbi written here, sines,
the scaling of the input, the post-processing against plain loops, and the downsampler against scipy's polyphase resampler."""
import importlib
import math

import numpy as np
import pytest

from alac.net_amd.fbank import KaldiFbank
from alac.net_amd.mfcc import KaldiMfcc

kp = importlib.import_module("alac.net_amd.kaldi_pitch")      # (the package's attribute of that name is the function)

RATE = 16000


def small(**kw):
    """The 36-state grid"""
    return kp.KaldiPitch(RATE, min_f0=100, max_f0=200, delta_pitch=0.02, **kw)


def sine(f, n, rate=RATE, amp=0.5):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / rate)).astype(np.float32)


def brute_force(nccf, spec, dtype=np.float64):
    """The cheapest path of nccf [2, T', S] by the plain recursion, no normalisation, every tie to the lowest source state and
    the first cheapest final state: (states, cost)"""
    T = spec.tables()
    sl, factor = T["sl"].astype(dtype), dtype(T["head"][0])
    n = nccf[0].astype(dtype)
    F, S = n.shape
    local = (1.0 - n) + sl[None, :] * n
    fwd, back = local[0].copy(), np.zeros((F, S), dtype=np.int64)
    for t in range(1, F):
        new = np.zeros(S, dtype=dtype)
        for i in range(S):
            best, arg = None, 0
            for j in range(S):
                c = fwd[j] + dtype((i - j) ** 2) * factor
                if best is None or c < best:
                    best, arg = c, j
            new[i], back[t, i] = best + local[t, i], arg
        fwd = new
    s = int(np.argmin(fwd))
    cost, path = float(fwd[s]), []
    for t in range(F - 1, -1, -1):
        path.append(s)
        s = int(back[t, s])
    return np.asarray(path[::-1]), cost


def test_the_lag_grid_and_the_integer_lags():
    spec = kp.KaldiPitch(RATE)
    lags = spec.lags()
    assert spec.n_states == 417 and len(lags) == 417 and (spec.first_lag, spec.last_lag) == (8, 82)
    assert lags[0] == 1 / 400 and lags[-1] <= 1 / 50 < lags[-1] * 1.005 and np.allclose(lags[1:] / lags[:-1], 1.005, rtol=1e-12)
    assert (spec.window, spec.shift, spec.win_length, spec.hop_length, spec.lines) == (100, 40, 400, 160, 3)
    assert small().n_states == 36 and kp.KaldiPitch(RATE, process=False).lines == 2
    t = spec.tables()
    assert t["down"].shape == (1, 17) and kp.KaldiPitch(44100).tables()["down"].shape == (40, 45)
    assert kp.KaldiPitch(22050).phases == 80
    first, up = t["up_first"], t["up"]
    assert first.min() >= 0 and (first + up.shape[1]).max() <= spec.n_lags
    with pytest.raises(ValueError):
        kp.KaldiPitch(44101)                                     # 4000 phases
    with pytest.raises(ValueError):
        kp.KaldiPitch(RATE, min_f0=20, delta_pitch=0.001)        # 2997 states
    with pytest.raises(ValueError):
        kp.KaldiPitch(RATE, snip_edges=False)


@pytest.mark.parametrize("kind", [KaldiFbank, KaldiMfcc])
def test_the_frame_count_is_the_feature_transform_s(kind):
    feat = kind(RATE)
    spec = kp.KaldiPitch.like(feat)
    assert spec.min_frames == feat.min_frames == 400 and spec.frames(399) == 0
    Ls = list(range(feat.min_frames, feat.min_frames + 2 * feat.hop_length + 1)) + [32000]
    assert [spec.frames(L) for L in Ls] == [feat.frames(L) for L in Ls]
    assert np.array_equal(spec.frames(np.asarray(Ls)), np.asarray([feat.frames(L) for L in Ls]))
    assert np.array_equal(spec.lengths(np.asarray([-1, 0, 399, 400, 32000])), [-1, 0, 0, 1, 198])
    # Kaldi's own count is one more where the last hop is all but complete: the track has the smaller one
    own = lambda L: 1 + (int(spec.samples(L)) - 100) // 40
    assert own(400 + 159) == 2 and spec.frames(400 + 159) == 1 and all(own(L) >= spec.frames(L) for L in Ls)
    with pytest.raises(ValueError):
        kp.KaldiPitch.like(kind(RATE, snip_edges=False))


def test_the_twin_is_within_the_nccf_bound_of_the_specification():
    rng = np.random.default_rng(1)
    x = np.stack([sine(140.0, 4000), (0.3 * rng.standard_normal(4000)).astype(np.float32),
                  np.concatenate([np.zeros(1500, np.float32), sine(220.0, 2500)])])[:, None]
    for spec in (kp.KaldiPitch(RATE), small(preemphasis=0.5)):
        _, info = kp.kaldi_pitch_host(x, spec, lengths=[4000, 3333, 4000], details=True)
        _, info32 = kp.kaldi_pitch_host_f32(x, spec, lengths=[4000, 3333, 4000], details=True)
        bound = kp.nccf_bound(spec, info)
        err = np.abs(info32["nccf"].astype(np.float64) - info["nccf"])
        finite = np.isfinite(bound)
        print("nccf: worst error", err[finite].max(), "worst finite bound", bound[finite].max(), "finite", finite.mean())
        assert finite[:, :, 0].all() and finite.mean() > 0.9      # the ballast keeps the pitch NCCF's root away from 0
        assert (err[finite] <= bound[finite]).all() and bound[finite].max() < 1e-2


def test_the_float32_path_costs_at_most_the_bound_more_than_the_optimum():
    spec = small(process=False)
    rng = np.random.default_rng(2)
    x = (sine(150.0, 400 + 39 * 160) + 0.2 * rng.standard_normal(400 + 39 * 160)).astype(np.float32)[None, None]
    _, info = kp.kaldi_pitch_host_f32(x, spec, details=True)
    nccf = info["nccf"]
    assert nccf.shape == (1, 1, 2, 40, 36)
    path, best = brute_force(nccf[0, 0].astype(np.float64), spec)
    got = kp.path_cost(nccf, info["states"], spec)[0, 0]
    assert abs(kp.path_cost(nccf, path[None, None], spec)[0, 0] - best) < 1e-9
    print("decode: float32 path", got, "optimum", best, "bound", kp.decode_bound(spec, 40))
    assert best - 1e-12 <= got <= best + kp.decode_bound(spec, 40)
    raw64, st64 = kp.kaldi_pitch_decode_host(nccf, spec, states=True)
    assert np.array_equal(st64[0, 0], path)                       # the float64 recursion is the brute force's, normalised


def test_sines_decode_within_the_bound():
    spec = kp.KaldiPitch(RATE, process=False)
    worst = 0.0
    for f in (80.0, 100.0, 125.0, 160.0, 200.0, 250.0, 333.0):
        n = 8000
        x = np.zeros((1, 1, n + 3200), dtype=np.float32)
        x[0, 0, 1600:1600 + n] = sine(f, n)
        y = kp.kaldi_pitch_host_f32(x, spec)[0, 0]
        # the frames whose whole span (25 ms and the longest lag) lies inside the sine
        t = np.arange(y.shape[1])
        inside = (t * 160 >= 1600) & (t * 160 + 4 * spec.span <= 1600 + n)
        assert inside.sum() >= 30
        cents = np.abs(1200.0 * np.log2(y[1, inside] / f))
        worst = max(worst, float(cents.max()))
        print(f"sine {f} Hz: worst {cents.max():.2f} cents, bound {kp.sine_bound_cents(spec, f):.2f}")
        assert cents.max() <= kp.sine_bound_cents(spec, f), f
    print("worst of all", worst)


def test_the_pov_feature_tells_a_sine_from_noise():
    spec = kp.KaldiPitch(RATE, add_normalized_log_pitch=False, add_delta_pitch=False)
    rng = np.random.default_rng(3)
    x = np.stack([sine(170.0, 8000), (0.5 * rng.standard_normal(8000)).astype(np.float32)])[:, None]
    y = kp.kaldi_pitch_host_f32(x, spec)
    assert y.shape == (2, 1, 1, 48)
    # Kaldi's POV feature falls as the NCCF rises: the sine's is below the noise's in every frame
    assert (y[0, 0, 0] < y[1, 0, 0]).all()
    raw = kp.kaldi_pitch_host_f32(x, kp.KaldiPitch(RATE, process=False))
    assert (raw[0, 0, 0] > raw[1, 0, 0]).all() and raw[0, 0, 0].min() > 0.9


def test_scaling_by_a_power_of_two_leaves_the_raw_track():
    spec = kp.KaldiPitch(RATE, process=False)
    rng = np.random.default_rng(4)
    x = (sine(130.0, 3000) + 0.1 * rng.standard_normal(3000)).astype(np.float32)[None, None]
    want = kp.kaldi_pitch_host_f32(x, spec)
    for k in (-20, -7, 3, 20):
        got = kp.kaldi_pitch_host_f32(np.ldexp(x, k).astype(np.float32), spec)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), k


def test_the_post_processing_against_plain_loops():
    spec = kp.KaldiPitch(RATE, normalization_left_context=2, normalization_right_context=2, add_raw_log_pitch=True)
    n = np.asarray([0.9, 0.2, -0.5, 0.99, 1.3, 0.0, 0.7])
    hz = np.asarray([100.0, 110.0, 120.0, 90.0, 200.0, 210.0, 150.0])
    raw = np.stack([n, hz])[None, None].astype(np.float32)
    y = kp.kaldi_pitch_process_host(raw, spec)[0, 0]
    y32 = kp.kaldi_pitch_process_host(raw, spec, f32=True)[0, 0]
    lp = np.log(hz)
    nc = np.clip(n.astype(np.float32).astype(np.float64), -1.0, 1.0)
    c = lambda v: float(np.float32(v))                            # the constants are float32 values in both host functions

    def pov(v):
        a = abs(v)
        r = c(-5.2) + c(5.4) * math.exp(c(7.5) * (a - 1)) + c(4.8) * a - 2 * math.exp(-10 * a) + c(4.2) * math.exp(20 * (a - 1))
        return 1 / (1 + math.exp(-r))

    for t in range(7):
        win = [u for u in range(t - 2, t + 3) if 0 <= u < 7]
        mean = sum(pov(nc[u]) * lp[u] for u in win) / sum(pov(nc[u]) for u in win)
        delta = sum(c(j / 10.0) * lp[min(max(t + j, 0), 6)] for j in range(-2, 3))
        want = [2 * ((c(1.0001) - nc[t]) ** c(0.15) - 1), 2 * (lp[t] - mean), 10 * delta, lp[t]]
        assert np.allclose(y[:, t], want, rtol=0, atol=1e-12), (t, y[:, t], want)
        # float32: the polynomials are good to 4 u of values up to 13.3 (log2 of 1e-4), the sums to a few u of 5.3
        assert np.allclose(y32[:, t], want, rtol=0, atol=2e-5), (t, y32[:, t], want)
    short = kp.kaldi_pitch_process_host(raw, spec, frame_counts=[3])[0, 0]
    assert not short[:, 3:].any() and short[:, :3].all()


@pytest.mark.parametrize("rate", [16000, 44100])
def test_the_downsampler_against_scipy(rate):
    signal = pytest.importorskip("scipy.signal")
    spec = kp.KaldiPitch(rate)
    T = spec.tables()
    rng = np.random.default_rng(5)
    x = rng.standard_normal(5000).astype(np.float32)
    got = kp._downsample(x, len(x), spec, T, np.float64)
    # the taps of resample_poly(up = P, down = I): the prototype h at the rate P fs, h[m] the weight of an input sample m / (P fs)
    # behind the output's time; phase ph's tap k lies (first_ph + k) P - ph I of those steps away
    P, I = spec.phases, spec.in_per_unit
    first, w = T["down_first"], T["down"].astype(np.float64)
    half = max(int(np.max(np.abs(first))), int(np.max(first + w.shape[1] - 1))) * P + I * P
    h = np.zeros(2 * half + 1)
    for ph in range(P):
        for k in range(w.shape[1]):
            h[half - ((first[ph] + k) * P - ph * I)] += w[ph, k]
    want = signal.resample_poly(x.astype(np.float64), P, I, window=h / P)             # (resample_poly scales its taps by `up`)
    n = min(len(got), len(want))
    assert abs(len(got) - len(want)) <= 1 and np.allclose(got[:n], want[:n], rtol=0, atol=1e-12)
