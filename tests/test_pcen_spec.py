"""pcen.py without a device: the specification against a literal loop and against scipy's lfilter, the smoothing coefficient,
the float32 twins against the specification within the derived bounds -- which a wrong gain or a wrong b leaves --, per-bin
parameters, every refusal of the constructor, what is not finite, and the entry point's declarations."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

from test_normalize_spec import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1e-6, 1.0, 2.0 ** 31)


def energies(shape, seed, scale=1.0):
    """Mel energies as a power spectrum gives them: chi-square with two degrees of freedom, the lines' levels spread over 11
    octaves, times `scale`"""
    rng = np.random.default_rng(seed)
    level = 2.0 ** rng.uniform(-11.0, 0.0, shape[:-1] + (1,))
    return (scale * level * rng.chisquare(2, shape)).astype(np.float32)


def literal(x, v, b, gain, bias, power, eps, scale):
    """One line in float64, as the issue writes it"""
    x = x.astype(np.float64)
    y = np.zeros(len(x))
    M = 0.0
    for t in range(v):
        s = scale * x[t]
        M = s if t == 0 else (1 - b) * M + b * s
        y[t] = (s / (eps + M) ** gain + bias) ** power - bias ** power
    return y


def f32(v):
    return float(np.float32(v))


def test_the_specification_is_the_literal_loop():
    from alac.net_amd.pcen import Pcen, pcen_host

    how = Pcen(0.06, gain=0.8, bias=1.5, power=0.25, eps=1e-5, scale=3.0)
    x = energies((3, 2, 5, 77), 1)
    lengths = [77, 40, -1]
    y = pcen_host(x, how, lengths)
    assert y.dtype == np.float64 and y.shape == x.shape
    for r, v in enumerate((77, 40, 0)):
        for c in range(2):
            for l in range(5):
                want = literal(x[r, c, l], v, f32(0.06), f32(0.8), f32(1.5), f32(0.25), f32(1e-5), f32(3.0))
                assert np.allclose(y[r, c, l], want, rtol=0, atol=1e-14), (r, c, l)      # (of values near 1.5^0.25: the difference cancels)
                assert (y[r, c, l, v:] == 0).all()
    assert np.array_equal(pcen_host(x, how), pcen_host(x, how, [77, 77, 99]))


def test_the_smoothing_coefficient_and_the_first_frame():
    from alac.net_amd.pcen import Pcen, pcen_smoother_host, smoothing_coefficient

    b = smoothing_coefficient(0.4, 100.0)
    assert abs(b - 0.024689453) < 5e-10 and b == (math.sqrt(1 + 4 * 40.0 ** 2) - 1) / (2 * 40.0 ** 2)
    assert Pcen(frame_rate=100.0).b == b and Pcen(frame_rate=50.0, time_constant=0.8).b == b
    x = energies((2, 3, 50), 2)
    M = pcen_smoother_host(x, Pcen(frame_rate=100.0, scale=2.0))
    assert np.array_equal(M[..., 0], 2.0 * x[..., 0].astype(np.float64))


def test_the_smoother_is_scipys_lfilter_from_its_steady_state():
    signal = pytest.importorskip("scipy.signal")
    from alac.net_amd.pcen import Pcen, pcen_smoother_host

    how = Pcen(frame_rate=100.0)
    x = energies((4, 300), 3)
    M = pcen_smoother_host(x, how)
    b = f32(how.b)
    zi = signal.lfilter_zi([b], [1, b - 1])
    for l in range(4):
        s = x[l].astype(np.float64)
        want, _ = signal.lfilter([b], [1, b - 1], s, zi=zi * s[0])
        assert np.allclose(M[l], want, rtol=1e-12, atol=0)


def yardstick(scale, seed=0, n=700):
    """The inputs the bound is held against: [3, 2, 8, n], both teams' line lengths by the caller's n"""
    return energies((3, 2, 8, n), 10 + seed, scale), [n, n // 2, n - 1]


@pytest.mark.parametrize("scale", SCALES)
def test_the_twin_is_within_the_bound_and_a_wrong_gain_or_b_is_not(scale):
    from alac.net_amd.pcen import Pcen, pcen_host, pcen_host_f32

    how = Pcen(frame_rate=100.0)
    for n in (700, 1300):                       # a wave's passes, a workgroup's
        x, lengths = yardstick(scale, n=n)
        y, dY = pcen_host(x, how, lengths, bound=True)
        got = pcen_host_f32(x, how, lengths).astype(np.float64)
        assert np.isfinite(y).all() and np.isfinite(dY).all()
        err = np.abs(got - y)
        assert (err <= dY).all(), float((err / dY).max())
        # the bound is relative to (s / (eps + M)^gain + bias)^power, and as tight as float32 allows: a few 1e-6 of it
        Wp = y + f32(how.bias) ** f32(how.power)
        on = np.broadcast_to(np.arange(n)[None, None, None, :] < np.asarray(lengths)[:, None, None, None], y.shape)
        assert (dY[on] / Wp[on]).max() < 2e-5
        # a plain float32 evaluation of the formulas stays within 1.6e-6 of that magnitude
        assert (err[on] / Wp[on]).max() < 1.6e-6
        # it is not vacuous: another gain leaves it by four orders of magnitude on nearly every frame; a b 5 % off -- which the
        # first frame, M[0] = s[0], and the frames where eps outweighs M (the scale of 1e-6) cannot show -- by three
        off = np.abs(pcen_host(x, Pcen(how.b, gain=0.97), lengths) - y)
        assert (off[on] > dY[on]).mean() > 0.99 and (off[on] / dY[on]).max() > 1e4 and (off[on] / Wp[on]).max() > 2e-2
        off = np.abs(pcen_host(x, Pcen(how.b * 1.05), lengths) - y)
        assert (off[on] > dY[on]).mean() > (0.4 if scale < 1.0 else 0.99) and (off[on] / dY[on]).max() > 1e3


def test_the_blocked_smoother_against_the_sequential_one():
    from alac.net_amd.pcen import Pcen, pcen_smoother_host, pcen_smoother_host_f32

    for b, n in ((0.024689453, 700), (0.5, 255), (1.0, 300), (0.003, 5000), (0.024689453, 2049)):
        how = Pcen(b, scale=1.5)
        x = energies((2, 3, n), n)
        lengths = [n, n - n // 3]
        M, dM = pcen_smoother_host(x, how, lengths, bound=True)
        blocked = pcen_smoother_host_f32(x, how, lengths)
        assert blocked.dtype == np.float32
        # the sequential float32 loop
        a32, b32 = np.float32(1.0) - np.float32(b), np.float32(b)
        s = (np.float32(1.5) * x).astype(np.float32)
        seq = np.zeros_like(x)
        for r, v in enumerate(lengths):
            m = s[r, :, 0]
            seq[r, :, 0] = m
            for t in range(1, v):
                m = ((a32 * m).astype(np.float32) + (b32 * s[r, :, t]).astype(np.float32)).astype(np.float32)
                seq[r, :, t] = m
        assert (np.abs(blocked - M) <= dM).all() and (np.abs(seq - M) <= dM).all(), (b, n)
        assert (np.abs(blocked.astype(np.float64) - seq) <= 2 * dM).all()
        # (a frame 1 / b back costs 3 / b roundings, the weights' mean: the bound is that many u of the line's largest M)
        assert (dM <= 1.02 * (3 / b + 35) * 2.0 ** -24 * np.abs(M).max(axis=-1, keepdims=True)).all()
        assert (blocked[1, :, lengths[1]:] == 0).all()
    # b = 1: M is s itself, in both
    x = energies((1, 2, 300), 5)
    assert same_bits(pcen_smoother_host_f32(x, Pcen(1.0)), x)


def test_per_bin_parameters_are_a_loop_over_scalar_specs():
    from alac.net_amd.pcen import Pcen, pcen_host, pcen_host_f32, pcen_smoother_host_f32

    L = 3
    b, gain, bias, power = [0.02, 0.05, 0.3], [0.98, 0.5, 0.0], [2.0, 0.0, 10.0], [0.5, 1.0, 0.125]
    how = Pcen(b, gain=gain, bias=bias, power=power, eps=1e-5)
    assert how.lines == L and how.table().shape == (5, L) and Pcen(0.1).lines is None
    x = energies((2, 2, L, 300), 6)
    lengths = [300, 170]
    y, y32, m32 = pcen_host(x, how, lengths), pcen_host_f32(x, how, lengths), pcen_smoother_host_f32(x, how, lengths)
    for l in range(L):
        one = Pcen(b[l], gain=gain[l], bias=bias[l], power=power[l], eps=1e-5)
        part = np.ascontiguousarray(x[:, :, l:l + 1])
        assert np.array_equal(pcen_host(part, one, lengths), y[:, :, l:l + 1])
        assert same_bits(pcen_host_f32(part, one, lengths), y32[:, :, l:l + 1])
        assert same_bits(pcen_smoother_host_f32(part, one, lengths), m32[:, :, l:l + 1])
    # mixed: a sequence and scalars
    mixed = Pcen(0.05, gain=[0.9, 0.8, 0.7])
    assert mixed.lines == 3 and mixed.table()[0].tolist() == [np.float32(0.05)] * 3
    for bad in (x[:, :, :2], x[:, 0], x[0]):
        with pytest.raises(ValueError):
            pcen_host(np.ascontiguousarray(bad), how)


def test_every_refusal_of_the_constructor_and_immutability():
    from alac.net_amd.pcen import Pcen

    for kw in (dict(), dict(b=0.1, frame_rate=100.0), dict(b=0.0), dict(b=-0.1), dict(b=1.5), dict(b=float("nan")), dict(b=float("inf")),
               dict(b=1e-50), dict(b=True), dict(b="0.1"), dict(frame_rate=0.0), dict(frame_rate=-1.0), dict(frame_rate=float("inf")),
               dict(frame_rate=100.0, time_constant=0.0), dict(frame_rate=100.0, time_constant=float("nan")),
               dict(b=0.1, gain=-0.1), dict(b=0.1, gain=float("inf")), dict(b=0.1, bias=-1.0), dict(b=0.1, bias=float("nan")),
               dict(b=0.1, power=0.0), dict(b=0.1, power=-0.5), dict(b=0.1, power=float("inf")), dict(b=0.1, power=1e-50),
               dict(b=0.1, eps=0.0), dict(b=0.1, eps=-1e-6), dict(b=0.1, eps=float("inf")), dict(b=0.1, eps=1e-50),
               dict(b=0.1, scale=0.0), dict(b=0.1, scale=-1.0), dict(b=0.1, scale=float("nan")), dict(b=0.1, scale=1e39),
               dict(b=[0.1, 0.2], gain=[0.5, 0.5, 0.5]), dict(b=[]), dict(b=[0.1, 0.0]), dict(b=0.1, gain=[0.5, -1.0]),
               dict(b=0.1, power=[[0.5]]), dict(b=0.1, bias=[1.0, float("nan")]), dict(b=0.1, eps=[1e-6])):
        with pytest.raises(ValueError):
            Pcen(**kw)
    with pytest.raises(TypeError):
        Pcen(0.1, 0.98)                                  # everything behind b goes by keyword
    how = Pcen(1.0, gain=0.0, bias=0.0)                  # the ends of the ranges are inside
    with pytest.raises(AttributeError):
        how.b = 0.5
    assert how == Pcen(1.0, gain=0.0, bias=0.0) and hash(how) == hash(Pcen(1.0, gain=0.0, bias=0.0)) and how != Pcen(1.0, gain=0.0)
    assert Pcen([0.1, 0.2]) == Pcen(np.array([0.1, 0.2])) and hash(Pcen([0.1, 0.2])) == hash(Pcen((0.1, 0.2)))


def test_like_takes_the_frame_rate_of_every_accepted_feature_spec():
    import alac.net_amd as pkg
    from alac.net_amd.pcen import Pcen, smoothing_coefficient

    for spec, rate in ((pkg.LogMel(16000, log=None), 100.0), (pkg.LogMel(22050, n_fft=1024, hop_length=256), 22050 / 256),
                       (pkg.KaldiFbank(16000, log=False), 100.0), (pkg.KaldiFbank(8000, win_length=200, hop_length=80), 100.0),
                       (pkg.ConstantQ(22050, log=None), 22050 / 512)):
        assert Pcen.like(spec).b == smoothing_coefficient(0.4, rate)
        assert Pcen.like(spec, time_constant=0.06, gain=0.8) == Pcen(frame_rate=rate, time_constant=0.06, gain=0.8)
    for bad in (pkg.KaldiMfcc(16000), pkg.Yin(16000), 16000, None):
        with pytest.raises(ValueError):
            Pcen.like(bad)
    with pytest.raises(ValueError):
        Pcen.like(pkg.LogMel(16000), b=0.1)
    assert pkg.Pcen is Pcen and pkg.normalize_host(energies((1, 2, 9), 0), Pcen(0.1)).shape == (1, 2, 9)


def test_what_is_not_finite_and_the_edges():
    from alac.net_amd.pcen import Pcen, pcen_host, pcen_host_f32, pcen_smoother_host_f32

    how = Pcen(frame_rate=100.0)
    for n in (300, 1100):
        v, at = n - 20, n // 3
        for bad in (np.nan, np.inf):
            x = energies((3, 2, n), 7)
            x[0, 1, at] = bad
            x[0, 0, v] = np.nan            # at v
            x[0, 0, n - 1] = np.inf        # behind v
            x[1] = np.nan                  # a length of -1: nothing of the row is read
            lengths = [v, -1, n]
            for fn in (pcen_host, pcen_host_f32, pcen_smoother_host_f32):
                # M is not finite from `at` on; behind an infinity s / inf^gain is 0 again and y is bias^power - c: IEEE's
                reached = np.zeros(n, dtype=bool)
                reached[at:at + 1 if bad == np.inf and fn is not pcen_smoother_host_f32 else v] = True
                y = fn(x, how, lengths)
                assert np.array_equal(~np.isfinite(y[0, 1]), reached), (fn.__name__, bad, n)
                if bad == np.inf and fn is not pcen_smoother_host_f32:
                    assert (np.abs(y[0, 1, at + 1:v]) < 1e-6).all()
                assert np.isfinite(y[0, 0]).all() and (y[0, :, v:] == 0).all() and (y[1] == 0).all() and np.isfinite(y[2]).all()
        # a NaN at v - 1 reaches that frame alone
        x = energies((1, 1, n), 8)
        x[0, 0, v - 1] = np.nan
        y = pcen_host_f32(x, how, [v])
        assert np.isnan(y[0, 0, v - 1]) and np.isfinite(y[0, 0, :v - 1]).all() and (y[0, 0, v:] == 0).all()
    # a negative energy: log2 of a negative number, NaN, in the specification and in the twin alike
    x = energies((1, 1, 40), 9)
    x[0, 0, 10] = -50.0
    y, t = pcen_host(x, how), pcen_host_f32(x, how)
    assert np.isnan(y[0, 0, 10]) and np.isnan(t[0, 0, 10]) and np.array_equal(np.isfinite(y), np.isfinite(t))
    # zeros throughout: bias^power - c, within one rounding of zero
    z = np.zeros((2, 3, 70), dtype=np.float32)
    for spec in (how, Pcen(0.1, bias=10.0, power=0.3), Pcen(0.1, bias=0.0)):
        y, dY = pcen_host(z, spec, bound=True)
        t = pcen_host_f32(z, spec)
        c = f32(spec.bias) ** f32(spec.power)
        assert (np.abs(y) <= 2.0 ** -24 * c).all() and (np.abs(t) <= 2.0 ** -22 * c).all() and (np.abs(t - y) <= dY).all()
    # lengths of 0 and 1, a line of one frame
    x = energies((2, 2, 1), 10)
    assert same_bits(pcen_smoother_host_f32(x, how, [1, 0]), np.stack([x[0], np.zeros_like(x[1])]))


def test_the_polynomials_are_within_their_stated_errors():
    from alac.net_amd.pcen import _DL, _EE, _exp2_f32, _log2_f32

    rng = np.random.default_rng(11)
    u = np.concatenate([rng.integers(1, 0x7F800000, 400000).astype(np.uint32).view(np.float32),
                        (1 + rng.uniform(-0.3, 0.5, 100000)).astype(np.float32),
                        np.array([1.0, 2.0, 0.5, 1.4142135, 1.4142137, 0.70710677, 0.7071068, 1e-45, 1e-39], dtype=np.float32)])
    want = np.log2(u.astype(np.float64))
    assert (np.abs(_log2_f32(u) - want) <= 2.0 ** -24 * np.abs(want) + _DL).all()
    assert _log2_f32(np.float32(1.0)) == 0 and _log2_f32(np.float32(8.0)) == 3 and _log2_f32(np.float32(2.0 ** -140)) == -140
    p = np.concatenate([rng.uniform(-126, 128, 400000).astype(np.float32), np.arange(-126, 128, dtype=np.float32)])
    want = np.exp2(p.astype(np.float64))
    assert (np.abs(_exp2_f32(p) - want) <= _EE * want).all()
    assert _exp2_f32(np.float32(10.0)) == 1024 and _exp2_f32(np.float32(-149.0)) == np.float32(2.0 ** -149)
    edge = np.array([0.0, -0.0, np.inf, -1.0, -np.inf, np.nan], dtype=np.float32)
    assert same_bits(_log2_f32(edge), np.array([-np.inf, -np.inf, np.inf, np.nan, np.nan, np.nan], dtype=np.float32))
    edge = np.array([128.0, np.inf, -150.5, -np.inf, np.nan, -150.0], dtype=np.float32)
    assert same_bits(_exp2_f32(edge), np.array([np.inf, np.inf, 0.0, 0.0, np.nan, 2.0 ** -150 * 0], dtype=np.float32))


def test_the_entry_is_declared_bound_and_in_the_csharp_binding():
    import alac.net_amd as pkg

    name = "alacgpu_pcen_device"
    header = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/alacgpu.h"
    n_args = len(m.group(1).split(","))
    restype, argtypes = pkg.SYMBOLS[name]
    assert n_args == 19 and restype is C.c_int and len(argtypes) == n_args
    m = re.search(r"extern\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", cs)
    assert m and len(m.group(1).split(",")) == n_args, f"{name} in AlacGpuNative.cs"
    assert getattr(pkg.lib(), name) and callable(pkg.AlacGpuContext.pcen_device)
    make = open(os.path.join(ROOT, "alac.net_amd", "csrc", "Makefile")).read()
    assert "alac_pcen.o" in re.search(r"^OBJS = (.*)$", make, re.M).group(1)
    # the module's constants are the header's
    from test_features import header_constant

    mod = importlib.import_module("alac.net_amd.pcen")           # (the package's `pcen` is the call)

    for const, value in (("ALAC_PCEN_CHUNK", mod.CHUNK), ("ALAC_PCEN_WAVE_MAX", mod.WAVE_MAX), ("ALAC_PCEN_LINE_THREADS", mod.LINE_THREADS),
                         ("ALAC_PCEN_TABLE_ROWS", 5)):
        assert header_constant(const, "alac_pcen.h") == value


def test_null_pointers_are_refused_without_a_device():
    import alac.net_amd as pkg

    BAD = int(re.search(r"ALACGPU_ERR_BAD_ARG\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "alacgpu.h")).read()).group(1))
    assert BAD == -1
    L = pkg.lib()
    p = C.c_void_p(4096)            # aligned, never dereferenced: the ctx is looked at first
    tail = (0.1, 0.98, 2.0, 0.5, 2.0 ** 0.5, 1e-6, 1.0, None, 0, 0, None)
    assert L.alacgpu_pcen_device(None, p, p, 1, 1, 8, 8, None, *tail) == BAD
    fake = C.c_void_p(8192)         # a ctx that is never dereferenced either: the pointers are looked at before it is used
    assert L.alacgpu_pcen_device(fake, None, p, 1, 1, 8, 8, None, *tail) == BAD
    assert L.alacgpu_pcen_device(fake, p, None, 1, 1, 8, 8, None, *tail) == BAD
