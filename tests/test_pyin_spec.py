"""pyin.py without a device: the tables against their definitions (and scipy's, where it is at hand), one frame's P_k against a
literal restatement of the module's steps 2 to 6, the float32 twin against the float64 specification within the module's two
bounds, the specification itself on sines and on a sine in noise, and every refusal of `PYin`."""
import json
import math
import os
import re

import numpy as np
import pytest

from test_yin_spec import mixed_signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 16000


def test_the_beta_weights():
    import alac.net_amd as pkg

    for beta, N in (((2, 18), 100), ((1, 1), 7), ((5, 3), 256), ((32, 32), 100)):
        w = pkg.PYin(RATE, beta=beta, n_thresholds=N).weights()
        assert w.shape == (N,) and (w >= 0).all() and abs(w.sum() - 1.0) <= 1e-12
    stats = pytest.importorskip("scipy.stats")
    for beta, N in (((2, 18), 100), ((5, 3), 256), ((32, 32), 100)):
        w = pkg.PYin(RATE, beta=beta, n_thresholds=N).weights()
        assert np.max(np.abs(w - np.diff(stats.beta.cdf(np.linspace(0, 1, N + 1), *beta)))) <= 1e-12


def test_the_boltzmann_factors():
    import alac.net_amd as pkg

    spec = pkg.PYin(RATE)
    t = spec.tables()
    for n in (1, 2, 5, spec.max_troughs):
        f = spec.boltzmann_factors(n)
        assert abs(f.sum() - 1.0) <= 1e-12
        assert np.allclose(t["bz"][:n].astype(np.float64) * float(t["inv"][n]), f, rtol=3 * 2.0 ** -24, atol=1e-45)
    stats = pytest.importorskip("scipy.stats")
    for l, n in ((2.0, 5), (0.5, 40), (2.0, 114)):
        assert np.max(np.abs(pkg.PYin(RATE, boltzmann=l).boltzmann_factors(n) - stats.boltzmann.pmf(np.arange(n), l, n))) <= 1e-12


def test_the_transition_rows_and_the_derived_sizes():
    import alac.net_amd as pkg

    for rate, hop, n_bins, h in ((16000, 160, 329, 40), (22050, 512, 329, 100), (8000, 80, 329, 40)):
        spec = pkg.PYin(rate, hop_length=hop)
        assert (spec.n_bins, spec.h, spec.nbps) == (n_bins, h, 10)
    for spec in (pkg.PYin(8000, 64, 80, 200.0, 800.0, resolution=0.5), pkg.PYin(8000, 64, 80, 200.0, 800.0, resolution=0.5, max_transition_rate=1.0),
                 pkg.PYin(8000, 64, 80, 200.0, 800.0, resolution=0.5, max_transition_rate=500.0), pkg.PYin(RATE)):
        T = spec.transition()
        n, h = spec.n_bins, spec.h
        assert T.shape == (n, n) and np.max(np.abs(T.sum(axis=1) - 1.0)) <= 1e-12
        o = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
        assert not T[o > h].any() and (T[o <= h] > 0).all()
        t = spec.tables()
        assert len(spec.table()) == sum(len(v) for v in t.values()) and len(t["lt"]) == spec.band + 1 == min(h, n - 1) + 1
        j, i = np.nonzero(o <= h)
        assert np.max(np.abs(2.0 ** (t["lt"][o[j, i]].astype(np.float64) - t["lz"][j]) - T[j, i])) <= 1e-6
        assert np.all(np.diff(t["edges"]) < 0) and np.all(np.diff(t["freq"]) > 0)
        assert abs(2.0 ** float(t["ls"][0]) + 2.0 ** float(t["ls"][1]) - 1.0) <= 1e-6


def restated(dp, spec):
    """Items 2 to 6 of the module for one frame, loop by loop: (lags, P_k, bins, vp)"""
    t = {k: v.astype(np.float64) for k, v in spec.tables().items()}
    N, l = spec.n_thresholds, spec.boltzmann
    taus = [tau for tau in range(spec.tau_min, spec.tau_max) if dp[tau] < dp[tau - 1] and dp[tau] <= dp[tau + 1]]
    m = [sum(1 for i in range(1, N + 1) if not dp[tau] < t["s"][i - 1]) for tau in taus]
    P = []
    for k in range(len(taus)):
        total = 0.0
        for i in range(m[k] + 1, N + 1):
            n_i = sum(1 for q in range(len(taus)) if m[q] < i)
            pos = sum(1 for q in range(k) if m[q] < i)
            total += t["beta"][i - 1] * (1.0 - math.exp(-l)) * math.exp(-l * pos) / (1.0 - math.exp(-l * n_i))
        P.append(total)
    if taus:
        least = min(range(len(taus)), key=lambda k: (dp[taus[k]], k))
        P[least] += float(np.float32(spec.no_trough_prob)) * sum(t["beta"][i - 1] for i in range(1, m[least] + 1))
    bins = []
    for tau in taus:
        a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
        shift = 0.5 * (a - c) / (a - 2 * b + c) if b <= a and b <= c and a - 2 * b + c > 0 else 0.0
        bins.append(sum(1 for e in t["edges"] if tau + shift < e))
    return taus, P, bins, min(sum(P), 1.0)


def test_one_frame_against_the_restated_steps():
    import alac.net_amd as pkg
    from alac.net_amd.yin import _dprime_f64, _segments

    spec = pkg.PYin(RATE)
    x = mixed_signal()
    _, info = pkg.pyin_host(x[None, :], spec, details=True)
    for t in (5, 12, 30):                      # in the tone, at its edge, in the noise
        dp = _dprime_f64(_segments(x, len(x), spec.yin, t, t + 1, np.float64), spec.yin)[0][0]
        taus, P, bins, vp = restated(dp, spec)
        got = info["troughs"][0][t]
        assert len(taus) >= 2 and list(got[0]) == taus and list(got[2]) == bins
        # (bz and inv are tables rounded to float32, the restatement's exponentials are not)
        assert np.allclose(got[1], P, rtol=4 * 2.0 ** -24, atol=0) and abs(float(info["vp"][0, t]) - vp) <= 4 * 2.0 ** -24


@pytest.fixture(scope="module")
def sines():
    """80, 150, 220 and 333 Hz, 0.5 s each with 0.1 s of silence behind each: (x, where each stretch lies, specification, twin)"""
    import alac.net_amd as pkg

    parts, where, at = [], [], 0
    for f in (80.0, 150.0, 220.0, 333.0):
        for n, hz in ((RATE // 2, f), (RATE // 10, 0.0)):
            parts.append(0.5 * np.sin(2 * np.pi * hz * np.arange(n) / RATE))
            where.append((at, at + n, hz))
            at += n
    x = np.concatenate(parts).astype(np.float32)[None, :]
    spec = pkg.PYin(RATE)
    return x, where, spec, pkg.pyin_host(x, spec, details=True), pkg.pyin_host_f32(x, spec, details=True)


def test_sines_and_silence(sines):
    """Every voiced frame whose span lies inside one sine is within 50 * resolution + 1 cents of the truth (half a bin, and 1
    cent for YIN's own measured 0.41), every frame whose span lies inside silence is unvoiced, and twin and specification
    decode the same states on every frame"""
    x, where, spec, (y, info), (y32, info32) = sines
    assert np.array_equal(info["states"], info32["states"])
    tol = 50.0 * spec.resolution + 1.0
    worst, inside = 0.0, 0
    for t in range(y.shape[-1]):
        s0 = spec.first + t * spec.hop_length
        for a0, a1, hz in where:
            if s0 >= a0 and s0 + spec.span <= a1:
                if hz == 0.0:
                    assert y[0, 1, t] == 0.0 and info["states"][0, t] >= spec.n_bins, t
                else:
                    assert y[0, 1, t] == 1.0, (t, "an unvoiced frame inside a sine")
                    worst, inside = max(worst, abs(1200.0 * math.log2(y[0, 0, t] / hz))), inside + 1
    print("worst", worst, "cents over", inside, "frames inside a sine; the tolerance is", tol)
    assert inside >= 150 and worst <= tol


def test_the_twin_is_within_the_bounds_of_the_specification(sines):
    import alac.net_amd as pkg
    from alac.net_amd.pyin import decode_bound, path_score, pk_bound, pk_floor, pyin_decode_host
    from alac.net_amd.yin import dprime_bound

    for x, spec, pair in ((sines[0], sines[2], (sines[3], sines[4])), (mixed_signal()[None, :], pkg.PYin(RATE, no_trough_prob=0.2), None)):
        (_, info), (_, info32) = pair or (pkg.pyin_host(x, spec, details=True), pkg.pyin_host_f32(x, spec, details=True))
        E, bound, checked = dprime_bound(spec.yin), pk_bound(spec), 0
        for t in range(info["margin"].shape[-1]):
            if info["margin"][0, t] > E:
                a, b = info["troughs"][0][t], info32["troughs"][0][t]
                assert np.array_equal(a[0], b[0]), t
                assert (np.abs(b[1].astype(np.float64) - a[1]) <= bound * a[1] + pk_floor(spec)).all(), t
                checked += len(a[0])
        assert checked >= 50
        # the float64 score of the float32 recursion's path against the float64 optimum, both on the twin's observations
        ov, ou = info32["obs_voiced"][:, None], info32["obs_unvoiced"][:, None]
        best = pyin_decode_host(ov, ou, spec)
        T = ov.shape[2]
        gap = path_score(ov, ou, best, spec) - path_score(ov, ou, info32["states"][:, None], spec)
        print("score gap", float(gap[0, 0]), "D(T')", decode_bound(spec, T))
        assert -1e-9 <= gap[0, 0] <= decode_bound(spec, T)


def test_pyin_is_no_worse_than_yin_in_noise():
    """A 200 Hz sine in white noise at 9 dB, where `yin_host` has far more than 5 % of its frames more than 50 cents off (an
    SNR found on the CPU: at 12 dB it has 1 of 101): `pyin_host` has no more such frames.  Both counts go to profiles/pyin.json."""
    import alac.net_amd as pkg

    t = np.arange(RATE) / RATE
    noise = np.random.default_rng(2014).standard_normal(RATE)
    tone = np.sin(2 * np.pi * 200.0 * t)
    g = math.sqrt(np.mean(tone ** 2) / np.mean(noise ** 2)) * 10.0 ** (-9.0 / 20.0)
    x = (0.3 * (tone + g * noise)).astype(np.float32)[None, :]
    off = lambda f0: int((np.abs(1200.0 * np.log2(f0 / 200.0)) > 50.0).sum())
    frames = int(pkg.Yin(RATE).frames(RATE))
    n_yin, n_pyin = off(pkg.yin_host(x, pkg.Yin(RATE))[0, 0]), off(pkg.pyin_host(x, pkg.PYin(RATE))[0, 0])
    print("frames more than 50 cents off: yin", n_yin, "pyin", n_pyin, "of", frames)
    assert n_yin >= 0.05 * frames and n_pyin <= n_yin
    path = os.path.join(ROOT, "profiles", "pyin.json")
    try:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["noise_200hz_9db"] = dict(frames=frames, yin_off_by_50_cents=n_yin, pyin_off_by_50_cents=n_pyin)
        with open(path, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    except OSError:
        pass                                   # (a read-only checkout: the counts are printed above)


def test_every_refusal():
    import alac.net_amd as pkg

    for kw in (dict(n_thresholds=0), dict(n_thresholds=257), dict(n_thresholds=1.5), dict(beta=(0, 2)), dict(beta=(2, 63)), dict(beta=(2.0, 18)),
               dict(beta=2), dict(beta=(1, 2, 3)), dict(boltzmann=0.0), dict(boltzmann=float("inf")), dict(resolution=0.0),
               dict(resolution=1.5), dict(max_transition_rate=-1.0), dict(switch_prob=0.0), dict(switch_prob=1.0), dict(no_trough_prob=-0.1),
               dict(no_trough_prob=1.1), dict(resolution=0.01, fmin=60.0, fmax=400.0), dict(win_length=100), dict(fmax=9000.0),
               dict(fmin=5.0), dict(center=False), dict(align_length=100), dict(hop_length=0)):
        with pytest.raises(ValueError):
            pkg.PYin(RATE, **kw)
    spec = pkg.PYin(RATE)
    with pytest.raises(AttributeError):
        spec.resolution = 0.5
    assert spec == pkg.PYin(RATE) and hash(spec) == hash(pkg.PYin(RATE)) and spec != pkg.PYin(RATE, switch_prob=0.02)
    like = pkg.PYin.like(pkg.LogMel(RATE, hop_length=200), resolution=0.5)
    assert isinstance(like, pkg.PYin) and like.hop_length == 200 and like.center and like.nbps == 2
    kaldi = pkg.PYin.like(pkg.KaldiFbank(RATE, win_length=400, hop_length=160))
    assert not kaldi.center and kaldi.align_length == 400 and kaldi.min_frames == 400 and kaldi.frames(400) == 1
    with pytest.raises(ValueError):
        pkg.PYin.like(pkg.Yin(RATE))
    with pytest.raises(ValueError):
        pkg.pyin_host(np.zeros((1, 100), dtype=np.float32), pkg.Yin(RATE))
    with pytest.raises(ValueError):
        pkg.pyin_host(np.zeros((1, 100)), spec)
    y = pkg.pyin_host_f32(np.zeros((2, 1, 500), dtype=np.float32), spec, [0, 500])
    assert y.shape == (2, 1, 3, 4) and not y[0, :, :, 1:].any() and not spec.voiced(y).any() and (y[1, 0, 0] == spec.tables()["freq"][0]).all()


def test_the_constants_and_the_entry_are_those_of_the_headers():
    import sys

    import alac.net_amd as pkg

    P = sys.modules["alac.net_amd.pyin"]
    h = open(os.path.join(ROOT, "alac.net_amd", "csrc", "alac_pyin.h")).read()
    m = re.search(r"ALAC_PYIN_MAX_BINS = (\d+)u, ALAC_PYIN_MAX_THRESHOLDS = (\d+)u", h)
    assert m and (int(m.group(1)), int(m.group(2))) == (P.MAX_BINS, P.MAX_THRESHOLDS)
    order = re.search(r"const float ([^;]*);\n\};", h).group(1).replace("*", "").replace(" ", "").split(",")
    assert tuple(order) == P._TABLE_ORDER
    name = "alacgpu_pyin_device"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alacgpu.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(rf"\b{name}\s*\(([^)]*)\)", header)
    assert m, f"{name} is not declared in include/alacgpu.h"
    n_args = len(m.group(1).split(","))
    assert len(pkg.SYMBOLS[name][1]) == n_args == 26 and hasattr(pkg.AlacGpuContext, "pyin_device")
    m = re.search(rf"\b{name}\s*\(([^)]*)\)", cs)
    assert m and len(m.group(1).split(",")) == n_args, f"{name} in AlacGpuNative.cs"
    assert pkg.lib().alacgpu_pyin_device(None, None, 1, 1, 8, 8, None, 16000, 64, 80, 20, 80, 0, 100, 49, 8, 0.0, *([None] * 6), 1, 0, None) == -1
