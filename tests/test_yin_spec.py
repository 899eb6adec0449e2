"""The YIN specification in numpy (alac.net_amd/yin.py), without a device: the arguments of `Yin`, its frame counts against the
feature transforms', the accuracy of `yin_host` on sines, the float32 twin against it within the bounds the module derives, the
degenerate rows, and the twin against itself under another batch and another tile."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 16000


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def default_spec():
    import alac.net_amd as pkg

    return pkg.Yin(RATE, 512, 160, 60, 400, 0.1)


def mixed_signal():
    """The issue's signal: a 150 Hz three-harmonic tone with vibrato, a gap, noise, a digital silence inside the gap"""
    n = np.arange(8000)
    ph = 2 * np.pi * np.cumsum(150 * (1 + 0.05 * np.sin(2 * np.pi * 5 * n / RATE))) / RATE
    x = (0.5 * np.sin(ph) + 0.3 * np.sin(2 * ph) + 0.2 * np.sin(3 * ph)).astype(np.float32)
    x[3000:4500] = 0
    x = (x + 0.02 * np.random.default_rng(0).standard_normal(8000)).astype(np.float32)
    x[4000:4300] = 0
    return x


def voiced_noise(B, C, T, rate, seed):
    """[B, C, T] float32: a tone of its own per plane between 130 and 330 Hz with a second harmonic, and noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    f = rng.uniform(130.0, 330.0, (B, C, 1))
    x = 0.4 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(4 * np.pi * f * t + 1.0) + 0.05 * rng.standard_normal((B, C, T))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def mixed():
    """(x, what yin_host returns with margin=True, what yin_host_f32 returns with taus=True), computed once"""
    import alac.net_amd as pkg

    x = mixed_signal()[None, :]
    spec = default_spec()
    return x, pkg.yin_host(x, spec, margin=True), pkg.yin_host_f32(x, spec, taus=True)


def test_argument_errors():
    import alac.net_amd as pkg

    Y = pkg.Yin
    s = Y(16000)
    assert (s.win_length, s.hop_length, s.tau_min, s.tau_max, s.span, s.center, s.align_length) == (512, 160, 40, 267, 779, True, None)
    assert Y(16000) == s and hash(Y(16000)) == hash(s) and Y(16000, threshold=0.2) != s
    with pytest.raises(AttributeError):
        s.threshold = 0.5
    bad = [dict(win_length=0), dict(win_length=100), dict(win_length=2112), dict(win_length=512.0),
           dict(fmax=9000.0),                                                  # tau_min 1
           dict(fmin=320.0, fmax=320.0),                                       # the lags 50 .. 50 leave nothing to search
           dict(fmin=315.0, fmax=320.0),                                       # 50 .. 51: tau_max is not above tau_min + 1
           dict(fmin=7.0),                                                     # tau_max 2286
           dict(threshold=0.0), dict(threshold=1.5), dict(threshold=-0.1), dict(hop_length=0), dict(center=False),
           dict(center=False, align_length=0), dict(align_length=400), dict(fmin=float("nan")), dict(fmax=float("inf")),
           dict(threshold=float("nan")), dict(fmin=1e39), dict(fmin=-60.0), dict(center=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            Y(16000, **kw)
    assert (Y(16000, fmin=310.0, fmax=320.0).tau_min, Y(16000, fmin=310.0, fmax=320.0).tau_max) == (50, 52)
    with pytest.raises(ValueError):
        Y(0)
    with pytest.raises(ValueError):
        Y(16000.0)
    assert Y(16000, 2048, fmin=7.8125).tau_max == 2048 and Y(16000, threshold=1.0).threshold == 1.0
    with pytest.raises(ValueError):
        Y(16000, fmin=7.8)


def test_frame_counts_and_like():
    import torch

    import alac.net_amd as pkg

    mel, fb, mf = pkg.LogMel(16000, n_fft=400, hop_length=160), pkg.KaldiFbank(16000, n_mels=23), pkg.KaldiMfcc(8000, win_length=200, hop_length=80)
    for s in (mel, fb, mf):
        y = pkg.Yin.like(s, fmin=80.0, threshold=0.2)
        assert (y.sample_rate, y.hop_length, y.fmin, y.threshold) == (s.sample_rate, s.hop_length, 80.0, 0.2)
        assert y.center == (s is mel) and y.align_length == (None if s is mel else s.win_length)
        hop, win = s.hop_length, getattr(s, "win_length", 0)
        edges = sorted({1, hop - 1, hop, hop + 1, max(win - 1, 1), win + 1 if win else 2, win + hop - 1, win + hop, 10 * hop, 10 * hop + win - 1,
                        10 * hop + win, s.min_frames, 32000})
        for L in edges:
            if L >= s.min_frames:
                assert y.frames(L) == s.frames(L), (s, L)
        assert np.array_equal(y.frames(np.array(edges)), [y.frames(L) for L in edges])
        lengths = torch.tensor([-1, 0, 1, hop - 1, hop, win - 1 if win else 3, win if win else 4, win + hop, 31999, 32000])
        assert torch.equal(y.lengths(lengths), s.lengths(lengths))
        assert np.array_equal(y.lengths(lengths.numpy()), s.lengths(lengths).numpy())
    assert pkg.Yin.like(mel).min_frames == 0 and pkg.Yin.like(fb).min_frames == 400
    with pytest.raises(ValueError):
        pkg.Yin.like(pkg.KaldiFbank(16000, snip_edges=False))
    with pytest.raises(ValueError):
        pkg.Yin.like(pkg.Deltas())


@pytest.mark.parametrize("f", [80.0, 110.0, 220.5, 333.0])
def test_the_specification_finds_a_sine_within_a_cent(f):
    """Measured while this was written: 0.03, 0.02, 0.08 and 0.41 cents"""
    import alac.net_amd as pkg

    spec = default_spec()
    x = np.sin(2 * np.pi * f * np.arange(8000) / RATE).astype(np.float32)
    y = pkg.yin_host(x[None, :], spec)
    assert y.shape == (1, 2, 51)
    inner = slice(6, 51 - 6)                                  # frames 6 .. T' - 7
    cents = np.abs(pkg.hz_to_cents(y[0, 0, inner], f))
    print(f, "Hz: within", cents.max(), "cents")
    assert cents.max() < 1.0 and spec.voiced(y)[0, inner].all()


def test_the_twin_is_within_the_derived_bounds_of_the_specification(mixed):
    """Measured while this was written: 51 frames, 35 voiced, no frame left out, the smallest margin 1.2e-3 against E = 7.7e-5,
    f0 2.6e-7 apart relatively, ap 5.8e-7 absolutely"""
    from alac.net_amd.yin import dprime_bound, f0_bound

    spec = default_spec()
    x, (y, tau, margin, kappa), (y32, tau32) = mixed
    E = dprime_bound(spec)
    assert 3e-5 < E < 1e-4
    assert y.shape == (1, 2, 51) and y32.dtype == np.float32 and int(spec.voiced(y).sum()) == 35 == int(spec.voiced(y32).sum())
    safe = margin[0] > E
    print("margins from", margin.min(), "E", E, "frames left out", int((~safe).sum()))
    assert (~safe).sum() <= 0.1 * safe.size
    assert np.array_equal(tau[0][safe], tau32[0][safe])
    f0, ap = y[0, 0][safe], y[0, 1][safe]
    df0 = np.abs(y32[0, 0][safe] - f0) / np.where(f0 == 0, 1.0, f0)
    dap = np.abs(y32[0, 1][safe] - ap)
    print("f0 relatively", df0.max(), "ap absolutely", dap.max())
    assert np.all(df0 <= f0_bound(spec, np.maximum(tau[0][safe], 1), kappa[0][safe]))
    assert np.all(dap <= E * ap)


def test_degenerate_rows():
    """Silence, a constant, v = 0, v < span // 2 and a NaN sample, in the specification and in the twin"""
    import alac.net_amd as pkg

    spec = default_spec()
    x = voiced_noise(5, 1, 3000, RATE, seed=1)[:, 0]
    x[0] = 0.0
    x[1] = -0.5
    lengths = [3000, 3000, 0, spec.span // 2 - 1, 3000]
    x[4, 1500] = np.nan
    y, tau, margin, _ = pkg.yin_host(x, spec, lengths, margin=True)
    y32, tau32 = pkg.yin_host_f32(x, spec, lengths, taus=True)
    n = spec.frames(3000)
    assert y.shape == y32.shape == (5, 2, n)
    for got in (y, y32):
        assert (got[0, 0] == 0).all() and (got[0, 1] == 1).all()                       # silence: every frame of the row
        assert (got[1, 0, 4:14] == 0).all() and (got[1, 1, 4:14] == 1).all()           # the constant, away from the row's ends
        assert got[1, 0, 0] > 0                                                       # (its first frame sees the step from zero)
        assert got[2, :, 0].tolist() == [0.0, 1.0] and not got[2, :, 1:].any()         # v = 0: one frame, of silence
        k = spec.frames(lengths[3])
        assert k == 3 and not got[3, :, k:].any() and (got[3, 0, :k] > 0).all()
        # the NaN: only frames whose span holds it, and there ap is NaN where every lag reaches it
        s = spec.first + np.arange(n) * spec.hop_length
        holds = (s <= 1500) & (1500 < s + spec.span)
        early = (s <= 1500) & (1500 < s + spec.win_length)
        assert not np.isnan(got[4][:, ~holds]).any() and np.isnan(got[4, 1, early]).all() and early.any()
        assert (got[4, 0, early] == np.float32(RATE) / spec.tau_min).all() and not spec.voiced(got)[4, early].any()
    clean = x.copy()
    clean[4, 1500] = 0.25
    assert same_bits(pkg.yin_host_f32(clean, spec, lengths)[4][:, ~holds], y32[4][:, ~holds])
    assert np.array_equal(tau[4][~np.isnan(y[4, 1])], tau32[4][~np.isnan(y[4, 1])])
    assert np.isinf(margin[0]).all() and np.isinf(margin[2]).all()


def test_the_twin_is_per_frame_not_per_tile_or_batch(mixed):
    import alac.net_amd as pkg
    from alac.net_amd.yin import tile_frames

    spec = default_spec()
    x, _, (y32, _) = mixed
    assert tile_frames(spec) == 8
    for tile in (1, 3, 51, 64):
        assert same_bits(pkg.yin_host_f32(x, spec, tile=tile), y32)
    other = voiced_noise(2, 1, 8000, RATE, seed=2)[:, 0]
    both = pkg.yin_host_f32(np.concatenate([other[:1], x, other[1:]]), spec, [8000, 5000, 8000], tile=5)
    assert same_bits(both[1], pkg.yin_host_f32(x, spec, [5000])[0])
    assert same_bits(pkg.yin_host_f32(x[:, None, :], spec), y32[:, None])
    # the tile of the kernel: fewer frames where a long hop or many lags would not fit
    assert tile_frames(pkg.Yin(16000, 2048, 160, 7.8125)) == 1 and tile_frames(pkg.Yin(16000, 512, 4000)) == 2
    assert tile_frames(pkg.Yin(16000, 64, 40, 125.0)) == 8


def test_the_tile_and_the_limits_are_the_header_s():
    import alac.net_amd.yin  # noqa: F401
    import sys

    Y = sys.modules["alac.net_amd.yin"]
    h = open(os.path.join(ROOT, "alac.net_amd", "csrc", "alac_yin.h")).read()
    for name, value in (("MIN_WIN", Y.MIN_WIN), ("MAX_WIN", Y.MAX_WIN), ("MAX_LAG", Y.MAX_LAG), ("TILE_MAX", Y.TILE_MAX),
                        ("LDS_FLOATS", Y.LDS_FLOATS)):
        m = re.search(rf"ALAC_YIN_{name} = (\d+)u", h)
        assert m and int(m.group(1)) == value, name


def test_the_entry_is_declared_bound_and_in_the_csharp_binding():
    import alac.net_amd as pkg

    name = "alacgpu_yin_device"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alacgpu.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(rf"\b{name}\s*\(([^)]*)\)", header)
    assert m, f"{name} is not declared in include/alacgpu.h"
    n_args = len(m.group(1).split(","))
    assert len(pkg.SYMBOLS[name][1]) == n_args == 17
    m = re.search(rf"\b{name}\s*\(([^)]*)\)", cs)
    assert m and len(m.group(1).split(",")) == n_args, f"{name} in AlacGpuNative.cs"
    assert pkg.hz_to_cents(np.array([200.0, 100.0]), 100.0).tolist() == [1200.0, 0.0]
