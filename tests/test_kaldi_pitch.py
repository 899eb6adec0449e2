"""alacgpu_kaldi_pitch_device on the GPU, bit for bit its float32 twin in numpy (kaldi_pitch.kaldi_pitch_host_f32): stage 0 and
every stage alone at 16 kHz and at 44.1 kHz (the multi-phase table), on 417 and on 36 states; the decode alone on hand-built
NCCFs against a brute-force Viterbi written in tests/test_kaldi_pitch_spec.py; slices, `out=` and canaries; the refusals."""
import importlib

import numpy as np
import pytest

from test_kaldi_pitch_spec import brute_force

pytestmark = pytest.mark.gpu

kp = importlib.import_module("alac.net_amd.kaldi_pitch")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def signals(B, C, T, rate, seed):
    """A sine, noise, a sine that starts mid-row, silence (rows cycle through them; the channels differ)"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    x = np.zeros((B, C, T), dtype=np.float32)
    for b in range(B):
        for c in range(C):
            kind = ([0, 1, 2, 3, 2, 3][b % 6] + c) % 4
            if kind == 0:
                x[b, c] = 0.4 * np.sin(2 * np.pi * (120.0 + 30 * c) * t)
            elif kind == 1:
                x[b, c] = 0.3 * rng.standard_normal(T)
            elif kind == 2:
                x[b, c, T // 2:] = 0.5 * np.sin(2 * np.pi * 180.0 * t[T // 2:])
    return x


GRID = [(16000, 6400, 1, dict()), (16000, 6400, 2, dict(min_f0=100, max_f0=200, delta_pitch=0.02)),
        (44100, 17640, 2, dict()), (44100, 17640, 1, dict(min_f0=100, max_f0=200, delta_pitch=0.02, preemphasis=0.5, add_raw_log_pitch=True))]


@pytest.mark.parametrize("rate,T,C,kw", GRID, ids=["16k-417", "16k-36-stereo", "44k-417-stereo", "44k-36-preemph"])
def test_the_kernels_equal_the_twin_bit_for_bit(rate, T, C, kw):
    import torch

    import alac.net_amd as pkg

    spec, plain = pkg.KaldiPitch(rate, **kw), pkg.KaldiPitch(rate, process=False, **kw)
    x = signals(6, C, T, rate, 7)                                 # rows 2 and 3 have no frame; 4 and 5 start mid-row and are silent
    lengths = [T, T - 1237, 0, spec.min_frames - 1, T, T - 100]
    d = torch.from_numpy(x).cuda()
    want, info = kp.kaldi_pitch_host_f32(x, spec, lengths, details=True)
    counts = info["frame_counts"]
    assert counts.tolist()[2:4] == [0, 0] and counts[0] == spec.frames(T) > counts[1] > 0
    got = pkg.kaldi_pitch(d, spec, lengths).cpu().numpy()
    assert got.shape == (6, C, spec.lines, spec.frames(T)) and np.array_equal(bits(got), bits(want))
    assert not got[2:4].any() and not got[1, :, :, counts[1]:].any()
    raw = pkg.kaldi_pitch(d, plain, torch.tensor(lengths)).cpu().numpy()
    assert np.array_equal(bits(raw), bits(info["raw"]))
    # every stage alone
    nccf = pkg.kaldi_pitch_nccf(d, spec, lengths)
    assert np.array_equal(bits(nccf.cpu().numpy()), bits(info["nccf"]))
    raw1 = pkg.kaldi_pitch_decode(nccf, spec, counts.tolist())
    assert np.array_equal(bits(raw1.cpu().numpy()), bits(info["raw"]))
    y = pkg.kaldi_pitch_process(raw1, spec, torch.from_numpy(counts).cuda())
    assert np.array_equal(bits(y.cpu().numpy()), bits(want))
    assert np.array_equal(bits(kp.kaldi_pitch_process_host(info["raw"], spec, counts, f32=True)), bits(want))


def hand_built(spec, F, kind, seed=0):
    rng = np.random.default_rng(seed)
    S = spec.n_states
    n = np.zeros((2, F, S), dtype=np.float32)
    if kind == "ties":                 # (the spec's soft_min_f0 is 0: local = 1 - n.)  Even frames: states 5 and 21 exactly as good;
        n[0, 0::2, 5] = n[0, 0::2, 21] = 0.5       # odd frames: state 13, as far from both -- a tie between its two sources in
        n[0, 1::2, 13] = 0.9                       # every odd frame, and between the two final states in the last
    elif kind == "jump":               # the best state moves from one end of the grid to the other half way
        n[0, :F // 2, 1] = 0.99
        n[0, F // 2:, S - 2] = 0.99
    else:
        n[0] = rng.uniform(-0.2, 0.9, (F, S))
    n[1] = rng.uniform(-1.0, 1.0, (F, S))
    return n.astype(np.float32)


def brute_force_rows(nccf, spec):
    """tests/test_kaldi_pitch_spec.py's brute force for long lines: the same plain recursion in float64 with no normalisation,
    every target's sources tried at once (np.argmin: the first, lowest source of a tie), written here, apart from the module"""
    T = spec.tables()
    sl, factor = T["sl"].astype(np.float64), float(T["head"][0])
    n = nccf[0].astype(np.float64)
    F, S = n.shape
    at = np.arange(S)
    trans = ((at[:, None] - at[None, :]) ** 2).astype(np.float64) * factor             # [target, source]
    local = (1.0 - n) + sl[None, :] * n
    fwd, back = local[0].copy(), np.zeros((F, S), dtype=np.int64)
    for t in range(1, F):
        new = np.zeros(S)
        for i in range(S):
            c = fwd + trans[i]
            back[t, i] = int(np.argmin(c))
            new[i] = c[back[t, i]] + local[t, i]
        fwd = new
    s = int(np.argmin(fwd))
    cost, path = float(fwd[s]), []
    for t in range(F - 1, -1, -1):
        path.append(s)
        s = int(back[t, s])
    return np.asarray(path[::-1]), cost


def plain_cost(pitch_nccf, path, spec):
    """The float64 cost of a path by a plain loop: the local costs and the transitions"""
    T = spec.tables()
    sl, factor = T["sl"].astype(np.float64), float(T["head"][0])
    total = 0.0
    for t, s in enumerate(path):
        n = float(pitch_nccf[t, s])
        total += (1.0 - n) + sl[s] * n + (factor * float((int(s) - int(path[t - 1])) ** 2) if t else 0.0)
    return total


@pytest.mark.parametrize("kind,F", [("ties", 9), ("jump", 12), ("random", 1), ("random", 2000)], ids=["ties", "jump", "one-frame", "2000-frames"])
def test_the_decode_alone_on_hand_built_nccfs(kind, F):
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiPitch(16000, min_f0=100, max_f0=200, delta_pitch=0.02, process=False, soft_min_f0=0 if kind == "ties" else 10)
    n = hand_built(spec, F, kind, F)
    nccf = np.stack([n, hand_built(spec, F, "random", F + 1)])[:, None]                    # [2, 1, 2, F, S]
    got = pkg.kaldi_pitch_decode(torch.from_numpy(nccf).cuda(), spec, [F, F - F // 3]).cpu().numpy()
    want, states = kp.kaldi_pitch_decode_host(nccf, spec, [F, F - F // 3], f32=True, states=True)
    assert np.array_equal(bits(got), bits(want)) and not got[1, 0, :, F - F // 3:].any()
    hz = spec.tables()["hz"]
    if F <= 12:                        # the brute force in float32, the kernel's roundings: the same path, ties and all
        path, _ = brute_force(nccf[0, 0], spec, np.float32)
        assert np.array_equal(path, states[0, 0]) and np.array_equal(got[0, 0, 1], hz[path])
        if kind == "jump":
            assert path[0] == 1 and path[-1] == spec.n_states - 2
        if kind == "ties":             # the lowest source, the first final state
            assert path.tolist() == [5, 13, 5, 13, 5, 13, 5, 13, 5]
    else:                              # the long walk back: the optimum is the brute force's, in float64 and without normalisation,
        for b, count in enumerate((F, F - F // 3)):          # per row up to its count
            path, best = brute_force_rows(nccf[b, 0, :, :count], spec)
            cost = kp.path_cost(nccf[b:b + 1, :, :, :count], states[b:b + 1, :, :count], spec)[0, 0]
            mine = plain_cost(nccf[b, 0, 0, :count], states[b, 0, :count], spec)
            print(f"row {b}: float32 path {mine}, optimum {best}, bound {kp.decode_bound(spec, count)}")
            assert abs(mine - cost) <= 1e-9 * count and best - 1e-9 <= mine <= best + kp.decode_bound(spec, count)
            assert abs(plain_cost(nccf[b, 0, 0, :count], path, spec) - best) <= 1e-9 * count
            assert np.array_equal(got[b, 0, 1, :count], hz[states[b, 0, :count]]) and (states[b, 0, count:] == -1).all()
            assert np.array_equal(got[b, 0, 0, :count], nccf[b, 0, 1, np.arange(count), states[b, 0, :count]])


def test_slices_and_out_write_nothing_else():
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiPitch(16000, min_f0=100, max_f0=200, delta_pitch=0.02)
    T = 3000
    x = signals(2, 2, T, 16000, 9)
    wide = torch.full((2, 2, T + 333), 7.0, device="cuda")
    wide[..., :T] = torch.from_numpy(x).cuda()
    want = kp.kaldi_pitch_host_f32(x, spec, [T, 2000])
    n = spec.frames(T)
    big = torch.full((4, 2, spec.lines, n), -3.0, device="cuda")
    out = pkg.kaldi_pitch(wide[..., :T], spec, [T, 2000], out=big[1:3])
    assert out.data_ptr() == big[1].data_ptr() and np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert bool((big[0] == -3.0).all()) and bool((big[3] == -3.0).all()) and bool((wide[..., T:] == 7.0).all())


def test_refusals_raise_and_write_nothing():
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiPitch(16000, min_f0=100, max_f0=200, delta_pitch=0.02)
    x = torch.zeros((2, 1, 3000), device="cuda")
    n = spec.frames(3000)
    out = torch.full((2, 1, spec.lines, n), -3.0, device="cuda")
    for bad in (lambda: pkg.kaldi_pitch(x.double(), spec), lambda: pkg.kaldi_pitch(x.cpu(), spec), lambda: pkg.kaldi_pitch(x, "spec"),
                lambda: pkg.kaldi_pitch(x, spec, out=out[:, :, :, :-1]), lambda: pkg.kaldi_pitch(x, spec, out=out[:1]),
                lambda: pkg.kaldi_pitch(x, spec, [1, 2, 3]), lambda: pkg.kaldi_pitch(x.view(2, 1, 4, 750)[:, :, 0], spec, out=x.view(-1)[:2 * spec.lines * spec.frames(750)].view(2, 1, spec.lines, spec.frames(750))),
                lambda: pkg.KaldiPitch(16000, min_f0=20, delta_pitch=0.001), lambda: pkg.KaldiPitch(44101),
                lambda: pkg.kaldi_pitch_process(torch.zeros((2, 1, 2, n), device="cuda"), pkg.KaldiPitch(16000, process=False)),
                lambda: pkg.kaldi_pitch_decode(torch.zeros((2, 1, 2, n, spec.n_states + 1), device="cuda"), spec)):
        with pytest.raises(ValueError):
            bad()
    assert bool((out == -3.0).all())
    # the C ABI refuses more than 1024 states and a table above what the launch holds, and writes nothing
    L = pkg.lib()
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as gpu:
        table = torch.zeros(1 << 16, device="cuda")
        a = lambda **kw: [{**dict(n_states=36, phases=1, down_taps=17), **kw}[k] for k in ("n_states", "phases", "down_taps")]
        for kw in (dict(n_states=1025), dict(phases=80, down_taps=52)):
            S, P, K = a(**kw)
            rc = L.alacgpu_kaldi_pitch_device(gpu._ctx, x.data_ptr(), 2, 1, 3000, 3000, None, 16000, 4000, 400, 160, 100, 40, 8, 82, S, P, 4, K, 10,
                                              15, 75, 75, 2, table.data_ptr(), None, None, out.data_ptr(), n, 0, None)
            assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
