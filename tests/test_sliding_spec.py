"""alac.net_amd/sliding.py without a device: the windows of `sliding_host` against a literal restatement of Kaldi's
SlidingWindowCmnInternal with running sums and against a table written out by hand; the float32 twin `sliding_host_f32`
within the derived bound dY of the specification, and a deliberately broken twin -- float32 prefix-sum differences and an
un-pivoted E[x^2] - m^2 -- far outside it; the degenerate cases; the argument checks of `SlidingMeanVar`; and the C ABI's
alacgpu_normalize_sliding_device: declared, bound, present in the C# binding, and its refusals, which need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_normalize_spec import dc, noise, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kaldi_restated(x, v, window, min_window, center, norm_vars):
    """Kaldi's SlidingWindowCmnInternal for one line x [n] float32 over its first v frames, in float64: the running sums of
    the window, the frames that enter added and the frames that leave subtracted.  Returns (y [v], s [v], e [v])."""
    x = x.astype(np.float64)
    y = np.zeros(v)
    ss, ee = np.zeros(v, dtype=np.int64), np.zeros(v, dtype=np.int64)
    cur_sum = cur_sumsq = 0.0
    last_start, last_end = -1, -1
    for t in range(v):
        if center:
            window_start = t - window // 2
            window_end = window_start + window
        else:
            window_start = t - window
            window_end = t + 1
        if window_start < 0:
            window_end -= window_start
            window_start = 0
        if not center:
            if window_end > t:
                window_end = max(t + 1, min_window)
        if window_end > v:
            window_start -= window_end - v
            window_end = v
            if window_start < 0:
                window_start = 0
        if last_start == -1:
            cur_sum = x[window_start:window_end].sum()
            cur_sumsq = (x[window_start:window_end] ** 2).sum()
        else:
            if window_start > last_start:
                assert window_start == last_start + 1
                cur_sum -= x[last_start]
                cur_sumsq -= x[last_start] ** 2
            if window_end > last_end:
                assert window_end == last_end + 1
                cur_sum += x[last_end]
                cur_sumsq += x[last_end] ** 2
        window_frames = window_end - window_start
        last_start, last_end = window_start, window_end
        ss[t], ee[t] = window_start, window_end
        y[t] = x[t] - cur_sum / window_frames
        if norm_vars:
            if window_frames == 1:
                y[t] = 0.0
            else:
                var = cur_sumsq / window_frames - (cur_sum / window_frames) ** 2
                y[t] *= max(var, 1e-10) ** -0.5
    return y, ss, ee


@pytest.mark.parametrize("window", [5, 8])
@pytest.mark.parametrize("center", [False, True])
def test_windows_against_kaldi_restated_with_running_sums(window, center):
    from alac.net_amd.sliding import SlidingMeanVar, sliding_host, sliding_windows

    n, checked = 44, 0
    x = noise((1, 1, n), 3 + window)
    for min_window in sorted({1, 3, window}):
        for norm_vars in (False, True):
            how = SlidingMeanVar(window, min_window, center, norm_vars)
            for v in sorted({1, 2, min_window - 1, min_window, window - 1, window, window + 1, 40} - {0}):
                got = sliding_host(x, how, [v])[0, 0]
                want, s, e = kaldi_restated(x[0, 0], v, window, min_window, center, norm_vars)
                gs, ge = sliding_windows(v, how)
                assert np.array_equal(gs, s) and np.array_equal(ge, e), (how, v)
                assert (got[v:] == 0).all()
                for t in range(v):
                    scale = np.abs(x[0, 0, s[t]:e[t]].astype(np.float64)).mean()
                    assert abs(got[t] - want[t]) <= 1e-10 * max(scale, 1e-30), (how, v, t, got[t], want[t])
                    checked += 1
    assert checked > 300


def test_the_windows_of_a_hand_written_table():
    """window 5, min_window 3, v 9: the non-centred window grows from min_window, is window + 1 = 6 frames long from frame 5
    on (Kaldi's quirk); the centred one is 5 frames and sticks to both ends"""
    from alac.net_amd.sliding import SlidingMeanVar, sliding_windows

    behind = [(0, 3), (0, 3), (0, 3), (0, 4), (0, 5), (0, 6), (1, 7), (2, 8), (3, 9)]
    around = [(0, 5), (0, 5), (0, 5), (1, 6), (2, 7), (3, 8), (4, 9), (4, 9), (4, 9)]
    for center, table in ((False, behind), (True, around)):
        s, e = sliding_windows(9, SlidingMeanVar(5, 3, center))
        assert list(zip(s.tolist(), e.tolist())) == table, center
    assert behind[8][1] - behind[8][0] == 5 + 1


def offset30(shape, seed):
    """30 + 1e-2 * noise: a feature with a large offset, such as c0"""
    return (30.0 + 1e-2 * noise(shape, seed).astype(np.float64)).astype(np.float32)


def broken_twin(x, how):
    """What the bound has to catch: float32 running prefix sums, a window sum as their difference, and E[x^2] - m^2 on the
    data as it is.  x [lines, n], whole lines."""
    from alac.net_amd.sliding import VAR_FLOOR, sliding_windows

    f32 = np.float32
    lines, n = x.shape
    c1, c2 = np.zeros((lines, n + 1), dtype=f32), np.zeros((lines, n + 1), dtype=f32)
    for i in range(n):
        c1[:, i + 1] = c1[:, i] + x[:, i]
        c2[:, i + 1] = c2[:, i] + (x[:, i] * x[:, i]).astype(f32)
    s, e = sliding_windows(n, how)
    fN = (e - s).astype(f32)
    m = ((c1[:, e] - c1[:, s]).astype(f32) / fN).astype(f32)
    y = (x - m).astype(f32)
    if how.norm_vars:
        var = np.maximum((((c2[:, e] - c2[:, s]).astype(f32) / fN).astype(f32) - (m * m).astype(f32)).astype(f32), VAR_FLOOR)
        y = (y / np.sqrt(var).astype(f32)).astype(f32)
    return y


def test_the_twin_is_within_the_bound_and_a_broken_twin_is_not():
    from alac.net_amd.sliding import SlidingMeanVar, sliding_host, sliding_host_f32

    for make, name in ((noise, "noise"), (offset30, "30 + 1e-2 noise")):
        for n, lengths in ((700, [700, 333, 0]), (300, [300, 257, 31])):
            x = make((3, 2, n), 11)
            for how in (SlidingMeanVar(), SlidingMeanVar.xvector(), SlidingMeanVar(300, 100, True, True),
                        SlidingMeanVar(33, 5, False, True), SlidingMeanVar(5, 1, True, False)):
                y, dY = sliding_host(x, how, lengths, bound=True)
                t = sliding_host_f32(x, how, lengths).astype(np.float64)
                err = np.abs(t - y)
                live = dY > 0
                print(f"{name} n {n} {how}: max err / dY {float((err[live] / dY[live]).max()):.4f}")
                assert (err <= dY).all(), (name, n, how, int(np.argmax(err - dY)))
    # teeth: n = 3000, window = 300 on 30 + 1e-2 noise
    x = offset30((1, 2, 3000), 5)
    for how in (SlidingMeanVar(300, 100, True, False), SlidingMeanVar(300, 100, False, True)):
        y, dY = sliding_host(x, how, bound=True)
        good = np.abs(sliding_host_f32(x, how).astype(np.float64) - y)
        bad = np.abs(broken_twin(x[0], how).astype(np.float64) - y[0])
        print(f"{how}: twin {float((good / dY).max()):.4f} of the bound, broken twin {float((bad / dY[0]).max()):.1f} of it")
        assert (good <= dY).all()
        assert (bad > dY[0]).mean() > 0.5, "the bound does not tell prefix-sum differences from window sums"


def test_degenerate_windows_and_lengths():
    from alac.net_amd.sliding import SlidingMeanVar, sliding_host, sliding_host_f32

    x = noise((4, 2, 50), 8)
    # N == 1 with norm_vars: window 1 centred, and a line of one valid frame
    for f in (sliding_host, sliding_host_f32):
        assert (f(x, SlidingMeanVar(1, 1, True, True)) == 0).all()
        assert (f(x, SlidingMeanVar(5, 1, False, True), [1, 1, 1, 1]) == 0).all()
        # v = 0 and a length of -1: zeros, and nothing of the row is read
        z = x.copy()
        z[1] = np.nan
        z[2] = np.inf
        got = f(z, SlidingMeanVar(5, 3, False, True), [50, 0, -1, 60])
        assert (got[1] == 0).all() and (got[2] == 0).all() and np.isfinite(got).all()
        # a constant window: the variance is floored at 1e-10, the result finite
        c = np.full((1, 1, 40), 7.25, dtype=np.float32)
        got = f(c, SlidingMeanVar(8, 3, True, True))
        assert np.isfinite(got).all() and (np.abs(got) <= 1e-2).all()
    assert same_bits(sliding_host_f32(x, SlidingMeanVar(5, 3)), sliding_host_f32(x, SlidingMeanVar(5, 3), [50, 50, 99, 50]))


def test_a_nan_reaches_exactly_the_frames_whose_window_holds_it():
    from alac.net_amd.sliding import SlidingMeanVar, sliding_host, sliding_host_f32, sliding_windows

    n, v, at = 80, 70, 33
    for how in (SlidingMeanVar(8, 3, False, False), SlidingMeanVar(8, 3, True, True), SlidingMeanVar(33, 5, True, False),
                SlidingMeanVar(30, 30, False, True)):
        s, e = sliding_windows(v, how)
        holds = np.zeros(n, dtype=bool)
        holds[:v] = (s <= at) & (at < e)
        assert holds.any() and not holds[:v].all()
        for bad in (np.nan, np.inf):
            x = dc((2, 3, n), 4)
            x[0, 1, at] = bad
            x[0, 2, v] = np.nan                # at v
            x[0, 2, n - 1] = np.inf            # behind v
            clean = x.copy()
            clean[0, 1, at] = 0.5
            y, dY = sliding_host(x, how, [v, n], bound=True)
            ref = sliding_host(clean, how, [v, n])
            t = sliding_host_f32(x, how, [v, n])
            for got in (y, t):
                assert np.array_equal(~np.isfinite(got[0, 1]), holds), (how, bad)
                rest = np.ones_like(got, dtype=bool)
                rest[0, 1] = False
                assert np.isfinite(got[rest]).all(), (how, bad, "another line or row")
            assert np.array_equal(y[0, 1][~holds], ref[0, 1][~holds]), (how, bad, "a frame whose window does not hold it")
            ok = np.isfinite(y)
            assert (np.abs(t.astype(np.float64)[ok] - y[ok]) <= dY[ok]).all(), (how, bad)


def test_sliding_meanvar_arguments_and_immutability():
    import alac.net_amd as pkg
    from alac.net_amd.sliding import SlidingMeanVar

    d = SlidingMeanVar()
    assert (d.window, d.min_window, d.center, d.norm_vars) == (600, 100, False, False)
    xv = SlidingMeanVar.xvector()
    assert (xv.window, xv.min_window, xv.center, xv.norm_vars) == (300, 100, True, False)
    assert pkg.SlidingMeanVar is SlidingMeanVar and xv == SlidingMeanVar(300, center=True) and hash(xv) == hash(SlidingMeanVar(300, 100, True))
    for kw in (dict(window=0), dict(window=-3), dict(window=2.0), dict(window=True), dict(min_window=0), dict(min_window=1.5),
               dict(window=5, min_window=6), dict(center=1), dict(norm_vars="yes"), dict(norm_vars=None)):
        with pytest.raises(ValueError):
            SlidingMeanVar(**kw)
    with pytest.raises(AttributeError):
        d.window = 3
    with pytest.raises(AttributeError):
        del d.center
    x = noise((2, 3, 20), 1)
    # normalize_host and normalize_host_f32 take it by handing it on
    assert np.array_equal(pkg.normalize_host(x, xv, [20, 7]), pkg.sliding_host(x, xv, [20, 7]))
    assert same_bits(pkg.normalize_host_f32(x, xv, [20, 7]), pkg.sliding_host_f32(x, xv, [20, 7]))
    for bad in ((x.astype(np.float64), xv), (x, pkg.MeanVar()), (x[0, 0], xv), (x, xv, [1]), (x, xv, [1.0, 2.0])):
        with pytest.raises(ValueError):
            pkg.sliding_host(*bad)
        with pytest.raises(ValueError):
            pkg.sliding_host_f32(*bad)


def test_vad_sits_in_front_of_augment_in_both_signatures():
    from alac.net_amd.corpus import Corpus

    for f in (Corpus.crops, Corpus.random_crops):
        names = list(inspect.signature(f).parameters)
        assert names.index("vad") == names.index("augment") - 1 == names.index("deltas") + 1, names
        assert names[-3:] == ["augment", "sample_rate", "mono"]
        assert inspect.signature(f).parameters["vad"].default is None


ENTRIES = ("alacgpu_normalize_sliding_device", "alacgpu_vad_energy_device", "alacgpu_select_frames_device")


def test_the_three_entries_are_declared_bound_and_in_the_csharp_binding():
    import alac.net_amd as pkg

    header = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/alacgpu.h"
        n_args = len(m.group(1).split(","))
        restype, argtypes = pkg.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args, (name, n_args, len(argtypes))
        m = re.search(r"extern\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", cs)
        assert m and len(m.group(1).split(",")) == n_args, f"{name} in AlacGpuNative.cs"
        assert getattr(pkg.lib(), name)
    for method in ("normalize_sliding_device", "vad_energy_device", "select_frames_device"):
        assert callable(getattr(pkg.AlacGpuContext, method))


def test_a_null_ctx_is_refused_without_a_device():
    import alac.net_amd as pkg

    BAD = int(re.search(r"ALACGPU_ERR_BAD_ARG\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "alacgpu.h")).read()).group(1))
    L = pkg.lib()
    p = C.c_void_p(4096)            # aligned, never dereferenced: the ctx is looked at first
    assert L.alacgpu_normalize_sliding_device(None, p, p, 1, 1, 8, 8, None, 5, 3, 0, 0, None) == BAD
    assert L.alacgpu_vad_energy_device(None, p, 1, 8, 0, 8, None, 5.0, 0.5, 0, 0.6, C.c_void_p(8192), 8, None) == BAD
    assert L.alacgpu_select_frames_device(None, p, p, 1, 1, 8, 8, None, C.c_void_p(8192), 8, C.c_void_p(12288), None) == BAD
