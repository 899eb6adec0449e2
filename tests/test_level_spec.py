"""The host side of the level stage (alac.net_amd/level.py), without a device: the twin against the specification within the
module's bound on the rows the kernel tests use, the designed K-weighting against BS.1770's printed table, EBU Tech 3341's
readings within +-0.1 LU with both gates shown to matter and, in its five-channel case 6, the surround weight, the rows that
stay as they are, max_peak, clamp and NaNs, what Level refuses, the keyword's place in both signatures, the C ABI entry and
the header's constants."""
import ctypes as C
import functools
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8209
RATES = (8000, 11025)
U32 = 2.0 ** -24


def mod():
    import alac.net_amd  # noqa: F401

    return sys.modules["alac.net_amd.level"]


def lengths_of(rate):
    hop = mod().hop_frames(rate)
    return np.array([-1, 0, 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5 * hop - 1, 4095, 4096, 4097, 8192, T])


@functools.lru_cache(maxsize=None)
def rows(rate):
    """The rows of the kernel tests: [12, 2, T] of noise at amplitudes from 1e-5 (below the absolute gate) to 0.5, the last two
    with a second half 40 dB down (the relative gate), one length each; read-only"""
    rng = np.random.default_rng(rate)
    amp = np.array([0.3, 0.3, 0.3, 0.2, 0.05, 0.5, 0.1, 1e-5, 0.02, 0.4, 0.25, 0.125])
    x = amp[:, None, None] * rng.standard_normal((12, 2, T))
    x[10:, :, T // 2:] *= 0.01
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x, lengths_of(rate)


def specs():
    L = mod().Level
    return {"peak": L.peak(0.5), "rms": L.rms(-25.0), "lufs": L.lufs(-23.0), "lufs-max-peak": L.lufs(-10.0, max_peak=0.9),
            "rms-clamp": L.rms(-3.0, clamp=True), "peak-max-peak": L.peak(2.0, max_peak=1.5, clamp=True)}


@functools.lru_cache(maxsize=None)
def reference(rate, name):
    """(s, g, E, P) of level_host and (y, g, E, P) of level_host_twin on rows(rate), computed once"""
    import alac.net_amd as pkg

    x, lens = rows(rate)
    spec = specs()[name]
    return pkg.level_host(x, spec, rate, lens, details=True), pkg.level_host_twin(x, spec, rate, lens, details=True)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", ["peak", "rms", "lufs", "lufs-max-peak", "rms-clamp", "peak-max-peak"])
def test_the_twin_is_within_the_bound_of_the_specification(rate, name):
    (s, g, E, P), (y, gt, Et, Pt) = reference(rate, name)
    rel = np.abs(gt / g - 1.0)
    print(f"{name} at {rate} Hz: max |g_twin / g_host - 1| = {rel.max():.3e}")
    assert np.array_equal(P, Pt) and np.all(rel <= U32)
    assert np.array_equal(g == 1.0, gt == 1.0)
    err = np.abs(y.astype(np.float64) - s)
    peak = np.abs(s).max(axis=(1, 2), keepdims=True)
    assert np.all(err <= U32 * np.abs(s) + U32 * peak)
    x, lens = rows(rate)
    measured = g != 1.0
    assert measured[len(lens) - 1] and not measured[0] and not measured[1]
    if name.startswith("lufs"):
        hop = mod().hop_frames(rate)
        assert not measured[lens < 4 * hop].any() and not measured[7] and measured[(lens >= 4 * hop) & (np.arange(12) != 7)].all()
        # the relative gate bites on the last row: its gated energy is above the plain mean of its blocks
        assert E[11] > 1.5 * (x[11].astype(np.float64) ** 2).mean()


# ITU-R BS.1770-4, table 1 and table 2: the two sections at 48 kHz as (b0, b1, b2, a1, a2)
BS1770_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                       [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])


def response_db(q, rate, f):
    z = np.exp(-2j * np.pi * f / rate)
    h = np.ones_like(z)
    for b0, b1, b2, a1, a2 in q:
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return 20.0 * np.log10(np.abs(h))


def test_the_designed_k_weighting_against_the_printed_table():
    lv = mod()
    f = np.geomspace(20.0, 20000.0, 2001)
    dev = np.abs(response_db(lv.kweight(48000), 48000.0, f) - response_db(BS1770_48K, 48000.0, f))
    print(f"the K-weighting at 48 kHz against BS.1770's table, 20 Hz .. 20 kHz: at most {dev.max():.4f} dB, at {f[dev.argmax()]:.0f} Hz; "
          f"at 997 Hz {np.interp(997.0, f, dev):.4f} dB")
    assert dev.max() <= lv.KWEIGHT_TABLE_DB                 # (measured, and stated in the module)
    assert np.interp(997.0, f, dev) <= 0.05                 # at the reference tone well inside EBU's 0.1 LU


RATE = 48000


def sine(db, seconds, channels=2, f=997.0, rate=RATE):
    t = np.arange(int(seconds * rate)) / rate
    return np.tile((10.0 ** (db / 20.0) * np.sin(2.0 * np.pi * f * t)).astype(np.float32), (channels, 1))


def ungated(x, rate):
    """-0.691 + 10 log10 of the mean of ALL block energies of one row, from the twin's hop sums"""
    lv = mod()
    hop = lv.hop_frames(rate)
    s = lv._measure(x[None], np.array([x.shape[1]]), hop, lv.kweight(rate), True)[2][0]
    nb = s.shape[1] - 3
    z = (s[:, 0:nb] + s[:, 1:nb + 1] + s[:, 2:nb + 2] + s[:, 3:nb + 3]) / (4 * hop)
    e = sum(lv.WEIGHTS[c] * z[c] for c in range(s.shape[0]))
    return -0.691 + 10.0 * np.log10(e.mean())


def test_ebu_tech_3341_readings():
    import alac.net_amd as pkg

    read = lambda x: float(pkg.loudness_host(x[None], RATE, twin=True)[0])
    got = read(sine(0.0, 5, channels=1))
    print("997 Hz at 0 dBFS in one channel:", got)
    assert abs(got - -3.01) <= 0.1
    for db in (-23.0, -33.0):                                # cases 1 and 2
        got = read(sine(db, 20))
        print(f"stereo sine at {db} dBFS:", got)
        assert abs(got - db) <= 0.1
    # case 3: wrong without the relative gate
    x = np.concatenate([sine(-36.0, 10), sine(-23.0, 60), sine(-36.0, 10)], axis=1)
    got, plain = read(x), ungated(x, RATE)
    print("case 3:", got, "ungated:", plain)
    assert abs(got - -23.0) <= 0.1 and abs(plain - -23.0) > 0.1
    # the absolute gate: a second half below -70 LUFS that the relative gate alone would let through (it would sit at the mean
    # of everything less 10 LU, -77.6).  Of the 100 blocks above the gate 97 are loud and three straddle the seam with 3/4, 1/2
    # and 1/4 of their frames loud and the rest 10 dB down: that is what a BS.1770 meter reads
    x = np.concatenate([sine(-65.0, 10), sine(-75.0, 10)], axis=1)
    want = -65.0 + 10.0 * np.log10((97 + (0.75 + 0.025) + (0.5 + 0.05) + (0.25 + 0.075)) / 100)
    got, plain = read(x), ungated(x, RATE)
    print("absolute gate:", got, "a meter's:", want, "ungated:", plain)
    assert abs(got - want) <= 0.1 and abs(plain - want) > 0.1
    # the sequential specification reads what the twin reads
    x = sine(-23.0, 0.6, rate=8000)
    a, b = pkg.loudness_host(x[None], 8000), pkg.loudness_host(x[None], 8000, twin=True)
    assert abs(float(a[0]) - float(b[0])) < 1e-9
    assert pkg.loudness_host(np.zeros((1, 1, 8000), dtype=np.float32), 8000)[0] == -np.inf


def test_ebu_tech_3341_case_6_and_the_surround_weight(monkeypatch):
    """An outside yardstick for the channel weights: EBU Tech 3341 case 6, 997 Hz at -28.0 dBFS in L and R, -24.0 in C and
    -30.0 in Ls and Rs (the channel order of alac_level.h), reads -23.0 +- 0.1 LUFS: 2 10^-2.8 + 10^-2.4 + 2 1.41 10^-3.0 =
    9.97e-3, less 3.01 dB for a sine's mean square, is -23.02.  With every weight 1.0 the same signal reads 0.37 LU less."""
    import alac.net_amd as pkg

    lv = mod()
    x = np.concatenate([sine(db, 5, channels=1) for db in (-28.0, -28.0, -24.0, -30.0, -30.0)])[None]
    by_hand = 10.0 * np.log10(2 * 10 ** -2.8 + 10 ** -2.4 + 2 * 1.41 * 10 ** -3.0) - 3.0103
    assert abs(by_hand - -23.0) <= 0.05
    got = float(pkg.loudness_host(x, RATE, twin=True)[0])
    monkeypatch.setattr(lv, "WEIGHTS", (1.0,) * 5)
    plain = float(pkg.loudness_host(x, RATE, twin=True)[0])
    print("EBU Tech 3341 case 6:", got, "with every weight 1.0:", plain)
    assert abs(got - -23.0) <= 0.1 and abs(plain - -23.0) > 0.1
    # the order is L, R, C, Ls, Rs: the centre's level in a surround channel reads otherwise
    monkeypatch.undo()
    assert abs(float(pkg.loudness_host(x[:, [0, 1, 3, 2, 4]], RATE, twin=True)[0]) - -23.0) > 0.1


def test_the_rows_that_stay_as_they_are():
    import alac.net_amd as pkg

    lv = mod()
    rate, hop = 8000, 800
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal((6, 2, 4000))).astype(np.float32)
    x[1] = 0.0                                              # P == 0
    x[3] *= np.float32(1e-5)                                # no block above the absolute gate
    lens = np.array([0, 4000, 4 * hop - 1, 4000, 4000, -3])
    for fn in (pkg.level_host, pkg.level_host_twin):
        y, g, E, P = fn(x, lv.Level.lufs(-23.0, clamp=True), rate, lens, details=True)
        assert list(g != 1.0) == [False, False, False, False, True, False]
        assert np.array_equal(np.asarray(y[[0, 1, 2, 3, 5]], dtype=np.float32).view(np.int32), x[[0, 1, 2, 3, 5]].view(np.int32))
        assert E[3] == 0.0 and E[1] == 0.0 and P[0] == 0.0 and P[3] > 0.0
        assert np.array_equal(np.asarray(y[4], dtype=np.float32)[:, 4000:].view(np.int32), x[4][:, 4000:].view(np.int32))
        # rms measures the short and the quiet rows; a peak target of exactly the peak is a gain of exactly 1
        y, g, E, P = fn(x, lv.Level.rms(-20.0), rate, lens, details=True)
        assert list(g != 1.0) == [False, False, True, True, True, False]
        assert abs(10 * np.log10((np.asarray(y[4], dtype=np.float64) ** 2).mean()) - -20.0) < 1e-3
        y, g, E, P = fn(x[4:5], lv.Level.peak(float(np.abs(x[4]).max())), rate, None, details=True)
        assert g[0] == 1.0 and np.array_equal(np.asarray(y, dtype=np.float32).view(np.int32), x[4:5].view(np.int32))
    # frames behind v are not measured: a loud tail changes nothing
    loud = x.copy()
    loud[4, :, 3500:] = 30.0
    a = pkg.level_host_twin(x, lv.Level.lufs(), rate, np.array([0, 0, 0, 0, 3500, 0]), details=True)
    b = pkg.level_host_twin(loud, lv.Level.lufs(), rate, np.array([0, 0, 0, 0, 3500, 0]), details=True)
    assert a[1][4] == b[1][4] != 1.0 and np.array_equal(b[0][4, :, 3500:], loud[4, :, 3500:])


def test_max_peak_clamp_and_nans():
    import alac.net_amd as pkg

    L = mod().Level
    rng = np.random.default_rng(6)
    x = (0.1 * rng.standard_normal((3, 1, 5000))).astype(np.float32)
    x[0, 0, 77] = 0.9
    for fn in (pkg.level_host, pkg.level_host_twin):
        free = fn(x, L.rms(-10.0), 8000, details=True)
        held = fn(x, L.rms(-10.0, max_peak=0.5), 8000, details=True)
        assert free[1][0] > held[1][0] == 0.5 / np.float64(np.float32(0.9)) and abs(np.abs(np.asarray(held[0][0], dtype=np.float64)).max() - 0.5) < 1e-7
        assert held[1][1] == free[1][1] or held[1][1] == 0.5 / free[3][1]
        hot = fn(x, L.rms(-3.0, clamp=True), 8000)
        assert np.abs(hot).max() == 1.0 and np.abs(np.asarray(fn(x, L.rms(-3.0), 8000))).max() > 1.0
        # a NaN below v is its own row's, one at or behind v is never read
        bad = x.copy()
        bad[1, 0, 100] = np.nan
        bad[2, 0, 4000] = np.inf
        y, g, E, P = fn(bad, L.rms(-10.0, clamp=True), 8000, np.array([5000, 5000, 4000]), details=True)
        clean = fn(x, L.rms(-10.0, clamp=True), 8000, np.array([5000, 5000, 4000]), details=True)
        assert np.isnan(g[1]) and np.isnan(P[1]) and np.isnan(y[1, 0, :5000]).all()
        assert g[0] == clean[1][0] and g[2] == clean[1][2] and np.array_equal(y[0], clean[0][0]) and y[2, 0, 4000] == np.inf
        assert np.array_equal(y[2, 0, :4000], clean[0][2, 0, :4000])
        # lufs: a NaN block is above no gate, and the NaN peak still limits nothing
        y, g, E, P = fn(bad, L.lufs(-20.0), 8000, details=True)
        assert np.isfinite(g[1]) and np.isnan(P[1]) and np.isnan(y[1, 0, 100]) and np.isfinite(y[1, 0, 101])


def test_what_level_refuses():
    import alac.net_amd as pkg

    L = pkg.Level
    for bad in (lambda: L.peak(0.0), lambda: L.peak(-1.0), lambda: L.peak(float("nan")), lambda: L.rms(float("inf")),
                lambda: L.lufs(float("nan")), lambda: L.lufs("loud"), lambda: L.lufs(True), lambda: L.rms(-25.0, max_peak=0.0),
                lambda: L.rms(-25.0, max_peak=float("nan")), lambda: L.rms(-25.0, clamp=1), lambda: L("vu", 1.0), lambda: L.rms(-4000.0),
                lambda: L.rms(4000.0)):
        with pytest.raises(ValueError):
            bad()
    a = L.lufs(-23.0)
    assert a == L.lufs() and hash(a) == hash(L.lufs()) and a != L.rms(-23.0) and a.linear == 10.0 ** ((-23.0 + 0.691) / 10.0)
    assert L.peak().target == 1.0 == L.peak().linear and L.rms().target == -25.0 and L.rms().linear == 10.0 ** -2.5
    with pytest.raises(AttributeError):
        a.target = 0.0
    x = np.zeros((1, 6, 4000), dtype=np.float32)
    for args in ((x, L.lufs(), 8000), (x[:, :2], L.lufs(), 150), (x[:, :2], L.lufs(), 3000), (x[:, :2], L.lufs(), None),
                 (x[:, :2], "lufs", 8000), (x[0], L.peak(), 8000), (x.astype(np.float64), L.peak(), 8000), (x[:, :2], L.lufs(), float("nan"))):
        for fn in (pkg.level_host, pkg.level_host_twin):
            with pytest.raises(ValueError):
                fn(*args)
    assert pkg.level_host(x, L.rms(), None).shape == x.shape            # six channels and no rate: rms takes them
    with pytest.raises(ValueError):
        pkg.level_host(x[:, :1], L.peak(), 8000, [1.5])


def test_level_sits_between_effects_and_deltas_in_both_signatures():
    from alac.net_amd.corpus import Corpus

    for f in (Corpus.crops, Corpus.random_crops):
        names = list(inspect.signature(f).parameters)
        assert names.index("level") == names.index("effects") + 1 == names.index("deltas") - 1, names
        assert names[-3:] == ["augment", "sample_rate", "mono"] and inspect.signature(f).parameters["level"].default is None


def test_the_entry_is_declared_bound_and_in_the_csharp_binding():
    import alac.net_amd as pkg

    name = "alacgpu_level_device"
    header = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/alacgpu.h"
    n_args = len(m.group(1).split(","))
    restype, argtypes = pkg.SYMBOLS[name]
    assert n_args == 18 and restype is C.c_int and len(argtypes) == n_args
    m = re.search(r"extern\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", cs)
    assert m and len(m.group(1).split(",")) == n_args
    assert getattr(pkg.lib(), name) and callable(pkg.AlacGpuContext.level_device)
    for n in ("Level", "level", "loudness", "level_host", "level_host_twin", "loudness_host"):
        assert hasattr(pkg, n), n
    # a NULL ctx is refused without a device, and no rows need nothing of it
    fn = pkg.lib().alacgpu_level_device
    args = dict(d_src=0x10000, d_out=0x20000, rows=3, channels=2, stride=16, frames=10, d_valid=0x40000, mode=2, hop=16, d_kweight=0x50000,
                target=1.0, max_peak=0.0, clamp=0, d_gain=0x60000, d_energy=None, d_peak=None, stream=None)
    assert fn(None, *args.values()) == -1 and fn(None, *dict(args, rows=0).values()) == -1
    page = C.create_string_buffer(4096)
    assert fn(C.addressof(page), *dict(args, rows=0).values()) == 0
    assert fn(C.addressof(page), *dict(args, rows=0, hop=15).values()) == -1


def test_the_constants_are_the_headers():
    from test_features import header_constant

    lv = mod()
    for c in ("PEAK", "RMS", "LUFS", "MAX_CHANNELS", "MIN_HOP", "HEAD", "PART", "MAX_PARTS", "BATCH"):
        assert getattr(lv, c) == header_constant("ALAC_LEVEL_" + c, "alac_level.h"), c
    assert lv.THREADS == header_constant("ALAC_LEVEL_THREADS", "alac_level.h") and lv.MODES == ("peak", "rms", "lufs")
    src = open(os.path.join(ROOT, "alac.net_amd", "csrc", "alac_level.h")).read()
    num = lambda name: float(re.search(name + r"\s*=\s*([0-9.e+-]+)\s*[;,]", src).group(1))
    assert num("ALAC_LEVEL_GATE_ABS") == lv.GATE_ABS and num("ALAC_LEVEL_GATE_REL") == lv.GATE_REL
    assert (num("ALAC_LEVEL_WEIGHT_FRONT"), num("ALAC_LEVEL_WEIGHT_SURROUND")) == (lv.WEIGHTS[0], lv.WEIGHTS[4]) and lv.WEIGHTS[:3] == (1.0,) * 3
    assert abs(lv.GATE_ABS / 10.0 ** ((-70.0 + 0.691) / 10.0) - 1.0) <= 2.0 ** -52
    assert [lv.hop_frames(r) for r in (8000, 11025, 16000, 44100, 48000, 22050)] == [800, 1103, 1600, 4410, 4800, 2205]
    for rate in (8000, 16000, 44100, 48000):
        import alac.net_amd as pkg

        q = lv.kweight(rate)
        assert q.shape == (2, 5) and np.array_equal(q[0], pkg.highshelf(rate, 1500.0, math.sqrt(0.5), 4.0))
        assert np.array_equal(q[1], pkg.highpass(rate, 38.0, 0.5))
