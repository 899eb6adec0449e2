"""The constant-Q specification (alac.net_amd/cqt.py) without a device: what the transform is (a sine lands in its bin at half
its amplitude, to the leakage of its negative-frequency image), linearity, the tables' invariance under doubling the rate and
f_min, the float32 twin inside the derived bound at every element, the lengths and frame counts, the refusals, the rule for
input that is not finite (per bin, not per frame), the work the kernel's tiling issues, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, FMIN = 2000, 50.0          # N_0 = 673 at 12 bins an octave


def small(pkg, **kw):
    args = dict(hop_length=64, f_min=FMIN, n_bins=30)
    args.update(kw)
    return pkg.ConstantQ(SR, **args)


def test_a_sine_lands_in_its_bin_at_half_its_amplitude():
    import alac.net_amd as pkg

    spec = small(pkg, scale=False, power=1)
    f, N = pkg.cqt_frequencies(spec), pkg.cqt_lengths(spec)
    L = 4096
    n = np.arange(L, dtype=np.float64)
    for k, A in ((0, 1.0), (7, 0.25), (29, 3.0)):
        x = (A * np.sin(2.0 * np.pi * f[k] * n / SR + 0.3)).astype(np.float32)
        out = pkg.cqt_host(x, spec)
        T = out.shape[-1]
        interior = [t for t in range(T) if t * 64 - N[0] // 2 >= 0 and t * 64 + N[0] <= L]      # every bin's taps inside the signal
        assert len(interior) > 10
        # x = A / 2i (e^{i th} - e^{-i th}): the first term gives A / 2 exactly (the window sums to its own sum), the second the
        # window's transform at 2 f_k, which is the leakage; the tables and the sine are float32 values: A 2^-22 covers both
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N[k]) / N[k])
        leak = abs(np.sum(w * np.exp(-4.0j * np.pi * f[k] * np.arange(N[k]) / SR))) / np.sum(w)
        tol = A / 2.0 * leak + A * 2.0 ** -22
        col = out[:, interior]
        assert (np.argmax(col, axis=0) == k).all()
        assert np.abs(col[k] - A / 2.0).max() <= tol, (k, np.abs(col[k] - A / 2.0).max(), tol)
        assert tol < 1e-3 * A


def test_linearity_and_power():
    import alac.net_amd as pkg

    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 1500)).astype(np.float32)
    spec = small(pkg)
    one = pkg.cqt_host(x, spec)
    assert np.array_equal(pkg.cqt_host(x * np.float32(4.0), spec), 4.0 * one)           # a power of two: exactly
    # 3 x is rounded to float32, each sample by 2^-24 of itself at most: |C(y) - 3 C(x)| <= 3 2^-24 max|x| sum|g_k|, and
    # sum|g_k| = sqrt(N_k) <= sqrt(673) for each of the two parts
    y = (x * np.float32(3.0)).astype(np.float32)
    assert np.allclose(pkg.cqt_host(y, spec), 3.0 * one, rtol=1e-12, atol=2 * 3 * 2.0 ** -24 * float(np.abs(x).max()) * 673 ** 0.5)
    two = pkg.cqt_host(x, small(pkg, power=2))
    assert np.allclose(two, one ** 2, rtol=1e-12)
    for log, fn in (("ln", np.log), ("log10", np.log10)):
        assert np.allclose(pkg.cqt_host(x, small(pkg, log=log, floor=0.5)), fn(np.maximum(one, 0.5)), rtol=1e-12)
    assert one.shape == (2, 30, 1 + 1500 // 64)
    assert pkg.cqt_host(x[0], spec).shape == (30, 24)


def test_doubling_rate_and_f_min_changes_no_table():
    import alac.net_amd as pkg

    for kw in (dict(), dict(bins_per_octave=36, n_bins=40, filter_scale=0.5), dict(scale=False)):
        a, b = small(pkg, **kw), pkg.ConstantQ(2 * SR, **dict(dict(hop_length=64, f_min=2 * FMIN, n_bins=30), **kw))
        assert np.array_equal(a.table, b.table) and np.array_equal(a.lens, b.lens)
    assert not small(pkg).table.flags.writeable and not small(pkg).lens.flags.writeable
    with pytest.raises(AttributeError):
        small(pkg).hop_length = 3


def test_the_twin_is_within_the_bound_at_every_element():
    import alac.net_amd as pkg

    rng = np.random.default_rng(2)
    x = (rng.standard_normal((2, 1300)) * np.array([[1.0], [1e-3]])).astype(np.float32)
    x[1, 700:] = 0
    for kw in (dict(), dict(power=2), dict(log="ln", floor=1e-3), dict(log="log10", power=2, floor=1e-6),
               dict(bins_per_octave=24, filter_scale=0.5, hop_length=37, scale=False)):
        spec = small(pkg, **kw)
        ref, bound = pkg.cqt_host(x, spec, bound=True)
        twin = pkg.cqt_host_f32(x, spec)
        assert twin.dtype == np.float32 and twin.shape == ref.shape == bound.shape
        assert np.isfinite(bound).all() and (bound >= 0).all()
        err = np.abs(twin.astype(np.float64) - ref)
        assert (err <= bound).all(), (kw, float((err / np.maximum(bound, 1e-300)).max()))
        print(kw, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))


def test_lengths_frames_and_configurations():
    import math

    import alac.net_amd as pkg
    from alac.net_amd.cqt import C1_HZ, MAX_TAPS, tile_frames

    spec = small(pkg)
    Q = 1.0 / (2.0 ** (1.0 / 12) - 1.0)
    N = pkg.cqt_lengths(spec)
    assert N[0] == 673 and list(N) == [math.ceil(Q * SR / (FMIN * 2.0 ** (k / 12))) for k in range(30)]
    assert np.allclose(pkg.cqt_frequencies(spec), FMIN * 2.0 ** (np.arange(30) / 12), rtol=1e-15)
    assert spec.frames(1) == 1 and spec.frames(63) == 1 and spec.frames(64) == 2 and spec.min_frames == 1 and spec.n_mels == 30
    assert list(spec.frames(np.array([0, 640]))) == [1, 11]
    for k in (0, 5, 16, 29):
        re, im = spec.kernel(k)
        assert re.shape == im.shape == (N[k],) and re.dtype == np.float32
        assert abs(float(np.sum(np.hypot(re, im))) - math.sqrt(N[k])) < 1e-3          # s_k sum(w) / sum(w)
    # the four configurations the layout must hold
    for args, n0 in (((16000,), 8228), ((22050,), 11339), ((44100,), 22678), ((22050, 512, C1_HZ, 252, 36), 34683)):
        big = pkg.ConstantQ(*args)
        assert int(big.lens[0]) == n0 <= MAX_TAPS and tile_frames(n0, 512) >= 8


def test_lengths_of_feature_rows():
    torch = pytest.importorskip("torch")
    import alac.net_amd as pkg

    got = small(pkg).lengths(torch.tensor([0, 63, 64, 1000, -1]))
    assert got.dtype == torch.int64 and got.tolist() == [1, 1, 2, 16, -1]


def test_refusals():
    import alac.net_amd as pkg

    bad = [dict(f_min=600.0, n_bins=12), dict(n_bins=0), dict(n_bins=513), dict(bins_per_octave=0), dict(bins_per_octave=97),
           dict(hop_length=0), dict(hop_length=(1 << 20) + 1), dict(hop_length=2.5), dict(filter_scale=0.0), dict(filter_scale=17.0),
           dict(filter_scale=float("nan")), dict(power=3), dict(power=0.5), dict(power=True), dict(log="db"), dict(floor=0.0),
           dict(floor=float("inf")), dict(f_min=0.0), dict(f_min=-1.0), dict(scale=1), dict(filter_scale=0.01, n_bins=40),      # (a shortest kernel of one tap)
           dict(f_min=1.0, n_bins=1),                       # N_0 = 33 635 fits; see below for one that does not
           ]
    for kw in bad[:-1]:
        with pytest.raises(ValueError):
            small(pkg, **kw)
    small(pkg, **bad[-1])
    with pytest.raises(ValueError, match="longest kernel"):
        small(pkg, f_min=0.9, n_bins=1)                      # N_0 = 37 372 > 36 864
    with pytest.raises(ValueError):
        pkg.ConstantQ(0)
    with pytest.raises(ValueError):
        pkg.cqt_host(np.zeros(8, dtype=np.float64), small(pkg))
    with pytest.raises(ValueError):
        pkg.cqt_host(np.zeros((2, 0), dtype=np.float32), small(pkg))
    with pytest.raises(ValueError):
        pkg.cqt_host_f32(np.zeros(8, dtype=np.float32), pkg.LogMel(16000))
    with pytest.raises(ValueError):
        pkg.Yin.like("cqt")
    y = pkg.Yin.like(small(pkg, hop_length=80), fmin=100.0, fmax=400.0)
    assert y.center and y.hop_length == 80 and y.sample_rate == SR and y.frames(1000) == small(pkg, hop_length=80).frames(1000)


def test_what_is_not_finite_stays_in_its_bins_own_taps():
    import alac.net_amd as pkg

    rng = np.random.default_rng(3)
    spec = small(pkg, hop_length=50)
    N = pkg.cqt_lengths(spec)
    x = rng.standard_normal(1200).astype(np.float32)
    t = np.arange(spec.frames(1200))
    for fn in (pkg.cqt_host, pkg.cqt_host_f32):
        clean = fn(x, spec)
        for i, v in ((600, np.nan), (0, np.inf), (1199, -np.inf), (337, np.nan)):
            y = x.copy()
            y[i] = v
            got = fn(y, spec)
            first = t[None, :] * 50 - (N // 2)[:, None]                               # [n_bins, T']: the first tap of (k, t)
            reached = (first <= i) & (i < first + N[:, None])
            assert reached.any() and not reached.all()
            assert not np.isfinite(got[reached]).any(), (fn.__name__, i)
            if np.isnan(v):
                assert np.isnan(got[reached]).all()
            assert np.array_equal(got[~reached].view(np.uint8), clean[~reached].view(np.uint8)), (fn.__name__, i)
            assert np.array_equal(np.isnan(got), np.isnan(pkg.cqt_host(y, spec))), (fn.__name__, i)       # an infinity is one where IEEE says so
            # per bin, not per frame: some frame holds both kinds
            assert (reached.any(axis=0) & ~reached.all(axis=0)).any()
    # the tap whose window weight is zero counts: n = 0 of bin 0 in frame 10
    y = x.copy()
    y[10 * 50 - N[0] // 2] = np.nan
    assert np.isnan(pkg.cqt_host(y, spec)[0, 10]) and np.isnan(pkg.cqt_host_f32(y, spec)[0, 10])
    assert np.isfinite(pkg.cqt_host(y, spec)[1, 10])


def test_the_work_the_tiling_issues():
    import alac.net_amd as pkg

    spec = pkg.ConstantQ(22050)
    total, rows = pkg.cqt_work(spec)
    assert total == int(pkg.cqt_lengths(spec).sum()) == 200481
    assert total <= rows <= 1.6 * total, rows / total          # blocks of 16 bins at 12 an octave: 1.49
    assert abs(16384 * spec.n_bins / total - 6.9) < 0.05        # the dense 16384-tap form
    print(f"issued / contained: {rows / total:.3f}; dense: {16384 * spec.n_bins / total:.2f}")
    # the table is what the rows say: 2 floats (re, im) a row
    assert spec.table.size == 2 * rows


def test_the_abi_declares_the_call():
    from test_features import header_constant

    import alac.net_amd as pkg
    from alac.net_amd import cqt as _fn  # noqa: F401  (the call; the module's constants below)
    from alac.net_amd.cqt import BLOCK_BINS, LDS_FLOATS, MAX_BINS, MAX_HOP, MAX_TAPS, TILE

    assert (header_constant("ALAC_CQT_BLOCK_BINS", "alac_cqt.h"), header_constant("ALAC_CQT_TILE", "alac_cqt.h"),
            header_constant("ALAC_CQT_MAX_TAPS", "alac_cqt.h"), header_constant("ALAC_CQT_MAX_BINS", "alac_cqt.h"),
            header_constant("ALAC_CQT_LDS_FLOATS", "alac_cqt.h")) == (BLOCK_BINS, TILE, MAX_TAPS, MAX_BINS, LDS_FLOATS)
    assert MAX_HOP == 1 << 20
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alacgpu.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(r"int\s+alacgpu_cqt_device\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 17
    m = re.search(r"alacgpu_cqt_device\s*\(([^)]*)\)", cs)
    assert m and len(m.group(1).split(",")) == 17
    assert len(pkg.SYMBOLS["alacgpu_cqt_device"][1]) == 17
