"""The resampler's host side (alac.net_amd/resample.py), without a device: the table and `resample_host` against a direct
evaluation of the closed form, the window arithmetic of crops at a target rate, and the argument checks."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(44100, 16000), (44100, 48000), (48000, 44100), (44100, 22050), (101, 97)]
Z, ROLLOFF = 6, 0.99


def closed_form(r, R, T):
    """H[j, s] = h(s / a - j / b) for every target frame j < ceil(b T / a) and every source frame s < T: float64, rounded to
    float32 and widened again.  s / a - j / b is taken as the exact integer s b - j a over a b."""
    g = np.gcd(r, R)
    a, b = r // g, R // g
    f = ROLLOFF * min(a, b)
    Ty = -(-b * T // a)
    j = np.arange(Ty, dtype=np.int64)[:, None]
    s = np.arange(T, dtype=np.int64)[None, :]
    t = f * ((s * b - j * a).astype(np.float64) / (a * b))
    v = np.pi * t
    sinc = np.where(t == 0, 1.0, np.sin(v) / np.where(t == 0, 1.0, v))
    h = (f / a) * sinc * np.cos(v / (2 * Z)) ** 2
    h[np.abs(t) >= Z] = 0.0
    return h.astype(np.float32).astype(np.float64), a, b


@pytest.mark.parametrize("r,R", PAIRS)
def test_resample_host_is_the_closed_form(r, R):
    from alac.net_amd.resample import resample_host, resample_table

    a, b, width, d0, w = resample_table(r, R)
    N = 2 * width + 1
    rng = np.random.default_rng(r + R)
    signals = [rng.standard_normal((3, T)) for T in (0, 1, a - 1, a + 1, 2 * a + 3 * width + 5)]
    # an impulse at every position of a period, behind one period of silence
    signals.append(np.eye(3 * a + width)[a:2 * a])
    for x in signals:
        T = x.shape[-1]
        H, a_, b_ = closed_form(r, R, T)
        assert (a_, b_) == (a, b)
        got = resample_host(x, r, R)
        assert got.shape == (x.shape[0], -(-b * T // a)) and got.dtype == np.float64
        want = x @ H.T
        bound = N * 2.0 ** -50 * (np.abs(x) @ np.abs(H).T)
        assert (np.abs(got - want) <= bound).all(), (r, R, T, float(np.abs(got - want).max()))
        assert T == 0 or np.abs(want).max() > 0
    # the magnitude sum the GPU tests' tolerance is built from
    x = signals[4]
    H, _, _ = closed_form(r, R, x.shape[-1])
    mag = resample_host(x, r, R, magnitude=True)
    assert np.allclose(mag, np.abs(x) @ np.abs(H).T, rtol=1e-12, atol=0)


@pytest.mark.parametrize("r,R", PAIRS + [(44100, 8000), (96000, 44100), (44100, 12000), (44100, 24000), (44100, 32000)])
def test_table_rows_hold_every_non_zero_weight(r, R):
    from alac.net_amd.resample import resample_table

    a, b, width, d0, w = resample_table(r, R)
    N = 2 * width + 1
    g = np.gcd(r, R)
    assert (a, b) == (r // g, R // g) and width == int(np.ceil(Z * a / (ROLLOFF * min(a, b))))
    assert d0.dtype == np.int32 and d0.shape == (b,) and w.dtype == np.float32 and w.shape == (b, N) and b * N < 7000
    assert d0[0] == -width and (np.diff(d0) >= 0).all() and d0.min() >= -width and (d0 + N).max() <= width + a
    # the closed form over more than a row can hold, phase by phase (one period: source frame s = d, target frame j = i)
    T = a + 2 * width + 8
    shift = width + 4
    f = ROLLOFF * min(a, b)
    i = np.arange(b, dtype=np.int64)[:, None]
    d = np.arange(T, dtype=np.int64)[None, :] - shift
    t = f * ((d * b - i * a).astype(np.float64) / (a * b))
    h = (f / a) * np.sinc(t) * np.cos(np.pi * t / (2 * Z)) ** 2
    h[np.abs(t) >= Z] = 0.0
    h = h.astype(np.float32)
    full = np.zeros_like(h)
    for k in range(b):
        full[k, d0[k] + shift:d0[k] + shift + N] = w[k]
    assert np.array_equal(full, h)                  # every non-zero weight is in its row, and a row's padding is zero
    assert (np.count_nonzero(w, axis=1) >= N - 3).all()


def test_resampled_length_and_short_signals():
    from alac.net_amd.resample import resample_host

    for r, R in PAIRS:
        g = np.gcd(r, R)
        a, b = r // g, R // g
        for T in (0, 1, 2, a - 1, a, a + 1, 1000):
            y = resample_host(np.ones(T), r, R)
            assert y.shape == (int(np.ceil(b * T / a)),) == (-(-b * T // a),)
    y = resample_host(np.ones(4000), 44100, 16000)
    assert np.abs(y[50:-50] - 1).max() < 1e-3       # a low-pass with unit gain
    x = np.random.default_rng(1).standard_normal((2, 2, 50))
    assert np.array_equal(resample_host(x, 44100, 44100), x)
    m = resample_host(x, 44100, 44100, mono=True)
    x32 = x.astype(np.float32)
    assert m.shape == (2, 1, 50) and np.array_equal(m[:, 0], ((x32[:, 0] + x32[:, 1]) * np.float32(0.5)).astype(np.float64))
    assert np.array_equal(resample_host(x[:, :1], 44100, 16000, mono=True), resample_host(x[:, :1], 44100, 16000))


@pytest.mark.parametrize("r,R", PAIRS)
def test_source_window_holds_every_tap(r, R):
    from alac.net_amd.resample import resample_table, source_window

    a, b, width, d0, w = resample_table(r, R)
    N = 2 * width + 1
    for L in sorted({1, 2, max(b - 1, 1), b, b + 1, 3 * b + 7, 1000}):
        Ls = source_window(0, L, a, b, width)[1]
        assert Ls == ((L - 1) // b + 2) * a + 2 * width
        for o in list(range(0, 3 * b + 2)) + [10 ** 9, 10 ** 9 + b - 1]:
            s0, Ls2 = source_window(o, L, a, b, width)
            assert Ls2 == Ls and s0 == (o // b) * a - width
            j = np.arange(o, o + L, dtype=np.int64)
            taps = ((j // b) * a + d0[j % b])[:, None] + np.arange(N)[None, :]
            assert taps.min() >= s0 and taps.max() < s0 + Ls, (o, L)


@pytest.mark.parametrize("r,R", PAIRS)
def test_a_crop_of_the_resampled_signal_is_the_resampled_window(r, R):
    from alac.net_amd.resample import apply_table, resample_host, resample_table, source_window

    table = resample_table(r, R)
    a, b, width = table[:3]
    rng = np.random.default_rng(3)
    for T in (5, 2 * a + 1, 6 * a + 17):
        x = rng.standard_normal((2, T))
        y = resample_host(x, r, R)
        Ty = y.shape[-1]
        for L in (1, b, 2 * b + 3):
            for o in sorted(o for o in {0, 1, b - 1, b, Ty // 2, max(Ty - L, 0), max(Ty - 1, 0), Ty} if o <= Ty):
                s0, Ls = source_window(o, L, a, b, width)
                origin = max(s0, 0)
                window = x[:, origin:min(origin + Ls, T)]
                got = apply_table(window, *table, origin=origin, first=o, num_frames=L)
                want = np.zeros((2, L))
                n = min(L, Ty - o)
                want[:, :n] = y[:, o:o + n]
                assert np.array_equal(got, want), (T, L, o)      # the same weights on the same frames in the same order


def test_table_cap_and_argument_errors():
    from alac.net_amd.resample import resample, resample_host, resample_table

    with pytest.raises(ValueError, match=r"a = 44100, b = 44099.*16384"):
        resample_table(44100, 44099)
    with pytest.raises(ValueError, match="16384"):
        resample_table(44100, 16001)
    for bad in (0, -1, 1.5, "44100", None, True, 44100.0):
        with pytest.raises(ValueError, match="positive integer"):
            resample_table(bad, 16000)
        with pytest.raises(ValueError, match="positive integer"):
            resample_table(44100, bad)
        with pytest.raises(ValueError):
            resample_host(np.zeros(4), 44100, bad)
    assert resample_table(np.int64(44100), np.int32(16000))[0] == 441
    with pytest.raises(ValueError):
        resample(np.zeros((2, 10), np.float32), 44100, 16000)      # not a device tensor


def test_the_default_arguments_leave_crops_as_they_were():
    import alac.net_amd as pkg

    for fn in (pkg.Corpus.crops, pkg.Corpus.random_crops):
        p = inspect.signature(fn).parameters
        assert p["sample_rate"].default is None and p["mono"].default is False
        assert list(p)[-2:] == ["sample_rate", "mono"]           # behind every argument there was
    assert list(inspect.signature(pkg.Corpus.crops).parameters)[:7] == ["self", "files", "frame_offsets", "num_frames", "dtype", "out", "check"]
    assert pkg.resample is pkg.resample.__globals__["resample"] and pkg.resample_host and pkg.resample_table and pkg.source_window


def test_resample_entry_is_declared_bound_and_refuses_null():
    import alac.net_amd as pkg

    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+alacgpu_resample_device\s*\(([^)]*)\)", src)
    assert m, "include/alacgpu.h does not declare alacgpu_resample_device"
    assert len(m.group(1).split(",")) == len(pkg.SYMBOLS["alacgpu_resample_device"][1]) == 17
    assert hasattr(pkg.lib(), "alacgpu_resample_device")
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    assert "alacgpu_resample_device(" in cs
    # a NULL ctx is refused before anything touches a device
    assert pkg.lib().alacgpu_resample_device(None, None, 1, 1, 0, None, None, None, 1, 1, 1, 1, None, None, 0, None, None) == -1
