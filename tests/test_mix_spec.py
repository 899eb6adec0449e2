"""The host side of the noise mix (alac.net_amd/mix.py): AddNoise, the float64 specification against a direct restatement in
numpy, the float32 twin against the derived bound dY, NaN containment, and the arguments of the entry point.  CPU only.

The twin criterion is tests/test_normalize_spec.py's: dY bounds every float32 evaluation in any order, so the twin has
r = max |twin - specification| / dY <= 1; the tests on the GPU hold the kernel to r_gpu <= 4 r_twin and to the twin's bits."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_normalize_spec import header_args, noise, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


class _Open:
    """What stands in for an alacgpu context in a Corpus that never saw a device"""

    def close(self):
        pass


@pytest.fixture
def hollow():
    """A Corpus object without a device behind it: open as far as AddNoise looks"""
    import alac.net_amd as pkg

    c = pkg.Corpus.__new__(pkg.Corpus)
    c._gpu, c._pinned = _Open(), None
    yield c
    c._gpu = None


def test_addnoise_refuses_what_it_cannot_draw_and_is_immutable(hollow):
    import alac.net_amd as pkg

    a = pkg.AddNoise(hollow, 10)
    assert a.noise is hollow and a.snr_db == (10.0, 10.0) and a.p == 1.0
    b = pkg.AddNoise(hollow, (5, 20.5), p=0.25)
    assert b.snr_db == (5.0, 20.5) and b.p == 0.25 and b == pkg.AddNoise(hollow, [5.0, 20.5], 0.25) and hash(b) == hash(pkg.AddNoise(hollow, (5, 20.5), 0.25))
    assert a != b and pkg.AddNoise(hollow, (3, 3)) == pkg.AddNoise(hollow, 3) and pkg.AddNoise(hollow, -5.0, p=0).p == 0.0
    for bad in (dict(snr_db=NAN), dict(snr_db=INF), dict(snr_db="10"), dict(snr_db=None), dict(snr_db=(1,)), dict(snr_db=(1, 2, 3)),
                dict(snr_db=(20, 5)), dict(snr_db=(0, INF)), dict(snr_db=(NAN, 3)), dict(snr_db=True), dict(snr_db=1e39),
                dict(snr_db=10, p=-0.1), dict(snr_db=10, p=1.5), dict(snr_db=10, p=NAN), dict(snr_db=10, p="1"), dict(snr_db=10, p=None)):
        with pytest.raises(ValueError):
            pkg.AddNoise(hollow, **bad)
    for bad in (None, "musan", 3, object()):
        with pytest.raises(ValueError):
            pkg.AddNoise(bad, 10)
    for name, value in (("p", 0.5), ("snr_db", (0.0, 1.0)), ("noise", None)):
        with pytest.raises(AttributeError):
            setattr(a, name, value)
        with pytest.raises(AttributeError):
            delattr(a, name)
    with pytest.raises(AttributeError):
        a.other = 1
    hollow._gpu = None                      # closed
    with pytest.raises(ValueError):
        pkg.AddNoise(hollow, 10)
    with pytest.raises(ValueError):
        a.draw(4, 100)


def restated(x, n, a, v, vn):
    """One row of the issue's arithmetic, written out again with loops: x [C, T], n [Cn, T] float32, a float; float64 [C, T]"""
    C, T = x.shape
    Cn = n.shape[0]
    v, vn = min(max(v, 0), T), min(max(vn, 0), T)
    y = x.astype(np.float64)
    if a == 0 or v == 0 or vn == 0:
        return y
    ps = sum(float(x[c, i]) ** 2 for c in range(C) for i in range(v)) / (C * v)
    pn = sum(float(n[c, i]) ** 2 for c in range(Cn) for i in range(vn)) / (Cn * vn)
    if pn == 0:
        return y
    g = float(a) * (ps / pn) ** 0.5
    if g == 0:
        return y
    for c in range(C):
        for i in range(v):
            y[c, i] = float(x[c, i]) + g * float(n[c % Cn, i % vn])
    return y


def test_the_specification_is_the_arithmetic_written_out():
    from alac.net_amd.mix import mix_host, mix_host_f32

    T = 23
    rows = [  # (v, vn, a, what)
        (23, 23, 0.5, ""), (17, 23, 1.0, ""), (23, 5, 0.25, ""), (23, 1, 2.0, ""), (17, 7, 0.1, ""), (0, 23, 1.0, ""), (-1, 23, 1.0, ""),
        (23, 0, 1.0, ""), (23, -1, 1.0, ""), (23, 23, 0.0, ""), (23, 23, 1.0, "pn0"), (23, 23, 1.0, "ps0"), (30, 40, 0.7, ""),
        (12, 23, -0.5, ""), (23, 9, 1.0, "pn0 behind vn")]
    B = len(rows)
    for C, Cn in ((1, 1), (2, 1), (2, 2)):
        x, n = noise((B, C, T), 10 * C + Cn), noise((B, Cn, T), 20 * C + Cn)
        for b, (v, vn, a, what) in enumerate(rows):
            if what == "pn0":
                n[b] = 0
            if what == "ps0":
                x[b] = 0
            if what == "pn0 behind vn":            # silent only where it counts: the frames behind vn are not the noise's
                n[b, :, :9] = 0
        ratio = np.array([r[2] for r in rows], dtype=np.float32)
        lengths, nlen = [r[0] for r in rows], [r[1] for r in rows]
        y = mix_host(x, n, ratio, lengths, nlen)
        t = mix_host_f32(x, n, ratio, lengths, nlen)
        assert y.dtype == np.float64 and y.shape == x.shape and t.dtype == np.float32
        for b, (v, vn, a, what) in enumerate(rows):
            want = restated(x[b], n[b], float(ratio[b]), v, vn)
            np.testing.assert_allclose(y[b], want, rtol=1e-13, atol=1e-13, err_msg=f"C {C} Cn {Cn} row {b}")
            k = min(max(v, 0), T)
            assert np.array_equal(y[b, :, k:], x[b, :, k:]) and same_bits(t[b, :, k:], x[b, :, k:]), (C, Cn, b, "behind v")
            unmixed = a == 0 or k == 0 or vn <= 0 or what in ("pn0", "ps0", "pn0 behind vn")
            assert np.array_equal(y[b], x[b]) == unmixed and same_bits(t[b], x[b]) == unmixed, (C, Cn, b)
        # without lengths: whole rows
        whole = [T] * B
        assert np.array_equal(mix_host(x, n, ratio), mix_host(x, n, ratio, whole, whole))
        assert same_bits(mix_host_f32(x, n, ratio), mix_host_f32(x, n, ratio, whole, whole))
    # the one noise channel goes into both channels of the signal; the repeated noise is the noise's first vn frames
    x, n = noise((1, 2, 10), 1), noise((1, 1, 10), 2)
    y = mix_host(x, n, [1.0], [10], [3])
    g = (y[0, 0, 0] - x[0, 0, 0]) / n[0, 0, 0]
    np.testing.assert_allclose(y[0] - x[0], g * np.stack([n[0, 0, np.arange(10) % 3]] * 2), rtol=1e-9, atol=1e-12)
    # the requested ratio is the achieved one: P(y - x) = a^2 Ps where the noise is not repeated
    x, n = noise((1, 2, 500), 3), 0.01 * noise((1, 2, 500), 4)
    y = mix_host(x, n, [10 ** (-15 / 20)], [400], [450])
    d = y[0, :, :400] - x[0, :, :400].astype(np.float64)
    got_db = 10 * np.log10((x[0, :, :400].astype(np.float64) ** 2).mean() / (d ** 2).mean())
    want_db = 10 * np.log10((n[0, :, :450].astype(np.float64) ** 2).mean() / (n[0, :, :400].astype(np.float64) ** 2).mean()) + 15
    assert abs(got_db - want_db) < 1e-5


def ratio_of(y32, y, dY):
    live = dY > 0
    return float(np.max(np.abs(y32.astype(np.float64) - y)[live] / dY[live])) if live.any() else 0.0


TWIN_INPUTS = [("full-scale noise", 1.0, 1.0), ("a signal 60 dB under the noise", 1e-3, 1.0)]


@pytest.mark.parametrize("tag,sx,sn", TWIN_INPUTS, ids=[t[0] for t in TWIN_INPUTS])
def test_the_twin_lies_inside_the_bound_and_the_bound_is_not_vacuous(tag, sx, sn):
    from alac.net_amd.mix import PART, mix_host, mix_host_f32

    T = 2 * PART + 77
    lengths, nlen = [T, T - 100, PART + 3, 5000, 0], [T, 1000, T, PART, T]
    ratio = np.array([1.0, 0.1, 10.0, 0.5, 1.0], dtype=np.float32)
    for C, Cn in ((1, 1), (2, 1), (2, 2)):
        x, n = (sx * noise((5, C, T), 5 + C)).astype(np.float32), (sn * noise((5, Cn, T), 7 + Cn)).astype(np.float32)
        y, dY = mix_host(x, n, ratio, lengths, nlen, bound=True)
        t = mix_host_f32(x, n, ratio, lengths, nlen)
        err = np.abs(t.astype(np.float64) - y)
        r = ratio_of(t, y, dY)
        print(f"{tag} C {C} Cn {Cn}: max err {err.max():.3e}, r {r:.4f}, max dY / |y| {np.max(dY[dY > 0] / np.abs(y[dY > 0]).clip(1e-30)):.3e}")
        assert np.isfinite(t).all() and np.isfinite(dY).all() and (err <= dY).all(), (tag, C, Cn, int(np.argmax(err - dY)))
        assert 0 < r <= 1
        # not vacuous: the bound is a relative one, some thousand u of what is added and one u of the result
        assert (dY <= 2.0 ** -24 * (np.abs(y) + 3 * (C * T + Cn * T) * np.abs(y - x.astype(np.float64)))).all()
        for b, k in enumerate(lengths):
            assert (dY[b, :, k:] == 0).all() and same_bits(t[b, :, k:], x[b, :, k:])
        assert (dY[4] == 0).all()


def test_what_is_not_finite_stays_in_its_row():
    from alac.net_amd.mix import mix_host, mix_host_f32

    T = 300
    x, n = noise((5, 2, T), 11), noise((5, 1, T), 12)
    ratio = np.array([0.5, 0.5, 0.5, 0.0, 0.5], dtype=np.float32)
    lengths, nlen = [200, 300, 250, 300, 300], [300, 100, 300, 300, 300]
    for fn in (mix_host, mix_host_f32):
        ref = fn(x, n, ratio, lengths, nlen)
        z, m = x.copy(), n.copy()
        z[0, 1, 200] = NAN              # at v: not read
        m[1, 0, 100] = INF              # at vn: not read
        m[3] = NAN                      # a == 0: the row's noise is not read
        assert same_bits(fn(z, m, ratio, lengths, nlen)[:, :, :200], ref[:, :, :200])
        got = fn(z, m, ratio, lengths, nlen)
        got[0, 1, 200] = ref[0, 1, 200]
        assert same_bits(got, ref)
        for bad in (NAN, INF):
            z, m = x.copy(), n.copy()
            z[0, 0, 7] = bad            # inside v of row 0
            m[2, 0, 299] = bad          # inside vn of row 2, behind its v
            got = fn(z, m, ratio, lengths, nlen)
            assert same_bits(got[[1, 3, 4]], ref[[1, 3, 4]]), bad
            if np.isnan(bad):
                assert np.isnan(got[0, :, :200]).all() and np.isnan(got[2, :, :250]).all()
            else:                       # Ps = inf: g = inf; Pn = inf: Ps / inf = 0, g = 0, the row stays
                assert not np.isfinite(got[0, :, :200]).any() and np.array_equal(got[2], x[2])
            assert np.array_equal(got[0, 1, 200:], x[0, 1, 200:]) and np.array_equal(got[2, :, 250:], x[2, :, 250:])
    # a ratio is data: NaN makes its row NaN, a negative one subtracts
    r2 = ratio.copy()
    r2[4] = NAN
    assert np.isnan(mix_host_f32(x, n, r2, lengths, nlen)[4]).all()
    np.testing.assert_allclose(mix_host(x, n, -ratio)[0] - x[0], -(mix_host(x, n, ratio)[0] - x[0]), rtol=1e-12)


def test_the_host_functions_refuse_what_is_not_a_batch():
    from alac.net_amd.mix import mix_host, mix_host_f32

    x, n = np.zeros((2, 2, 8), dtype=np.float32), np.zeros((2, 1, 8), dtype=np.float32)
    for fn in (mix_host, mix_host_f32):
        for args in ((x.astype(np.float64), n, [1, 1]), (x, n.astype(np.float64), [1, 1]), (x[0], n[0], [1, 1]), (x, n[:1], [1, 1]),
                     (x, n[:, :, :7], [1, 1]), (x, np.zeros((2, 3, 8), dtype=np.float32), [1, 1]), (x, n, [1.0]), (x, n, 1.0),
                     (x, n, ["a", "b"]), (x, n, [1, 1], [8]), (x, n, [1, 1], [8.0, 8.0]), (x, n, [1, 1], None, [8, 8, 8])):
            with pytest.raises(ValueError):
                fn(*args)


def test_the_entry_point_is_declared_bound_and_exported():
    import alac.net_amd as pkg

    name = "alacgpu_mix_device"
    assert len(header_args(name)) == len(pkg.SYMBOLS[name][1]) == 14
    assert hasattr(pkg.lib(), name)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(r"extern\s+int\s+" + name + r"\s*\(([^)]*)\)", cs)
    assert m and len(m.group(1).split(",")) == 14
    for n in ("AddNoise", "mix", "mix_host", "mix_host_f32"):
        assert hasattr(pkg, n)
    assert hasattr(pkg.AlacGpuContext, "mix_device")
    from test_features import header_constant
    import importlib

    mix = importlib.import_module("alac.net_amd.mix")         # (the package's attribute of that name is the function)
    for c in ("PART", "MAX_PARTS", "ROUND", "VEC"):
        assert getattr(mix, c) == header_constant("ALAC_MIX_" + c, "alac_mix.h"), c
    assert mix._THREADS == header_constant("ALAC_MIX_THREADS", "alac_mix.h")


# A call's arguments in the header's order.  The pointers are numbers: an argument check never follows one, and every case
# below returns from the check -- a call that passed it would use the ctx, which here is a page of zeros.
SRC, OUT, NOISE, VALID, NVALID, RATIO = 0x10000, 0x20000, 0x30000, 0x40000, 0x40100, 0x40200
MIX = dict(d_src=SRC, d_out=OUT, d_noise=NOISE, rows=3, channels=2, noise_channels=1, stride=16, noise_stride=12, frames=10,
           d_valid=VALID, d_noise_valid=NVALID, d_ratio=RATIO, stream=None)
EXTENT, NOISE_EXTENT = 4 * (5 * 16 + 10), 4 * (2 * 12 + 10)
FAR = dict(d_src=2 ** 40, d_out=2 ** 46, d_noise=2 ** 50)       # arrays of 2^31 rows that still lie apart
CASES = [dict(d_src=None), dict(d_out=None), dict(d_noise=None), dict(d_ratio=None),
         dict(d_src=SRC + 2), dict(d_out=OUT + 1), dict(d_noise=NOISE + 2), dict(d_ratio=RATIO + 2), dict(d_valid=VALID + 4),
         dict(d_noise_valid=NVALID + 4), dict(channels=0), dict(noise_channels=0), dict(noise_channels=3),
         dict(channels=3, noise_channels=2), dict(frames=0), dict(frames=17, noise_stride=32), dict(frames=13), dict(stride=9),
         dict(d_out=SRC + 4), dict(d_out=SRC + EXTENT - 4), dict(d_src=OUT + EXTENT - 4), dict(d_out=SRC + 64),
         dict(d_noise=OUT), dict(d_noise=OUT + EXTENT - 4), dict(d_out=NOISE + NOISE_EXTENT - 4), dict(d_out=SRC, d_noise=SRC),
         dict(d_out=SRC, d_noise=SRC + EXTENT - 4),
         dict(rows=2 ** 32 - 1, channels=2 ** 32 - 1, noise_channels=1, stride=2 ** 40, frames=2 ** 40, noise_stride=2 ** 40),
         dict(rows=2 ** 20, channels=1, noise_channels=1, stride=10, frames=10, noise_stride=2 ** 40),
         dict(FAR, rows=2 ** 31, channels=1),                                                    # a workgroup per row
         dict(FAR, rows=2 ** 30, channels=1, stride=4097, noise_stride=4097, frames=4097)]      # two parts per row


def call(pkg, ctx, **kw):
    return pkg.lib().alacgpu_mix_device(ctx, *dict(MIX, **kw).values())


@pytest.mark.parametrize("change", CASES, ids=[f"{'-'.join(c)}-{i}" for i, c in enumerate(CASES)])
def test_bad_arguments_are_refused_before_anything_is_enqueued(change):
    import alac.net_amd as pkg

    page = ctypes.create_string_buffer(4096)
    assert call(pkg, ctypes.addressof(page), **change) == -1, change


def test_a_null_ctx_is_refused_and_no_rows_are_no_work():
    import alac.net_amd as pkg

    page = ctypes.create_string_buffer(4096)
    assert call(pkg, None) == -1                                              # every other argument is valid
    assert call(pkg, None, rows=0) == -1
    ctx = ctypes.addressof(page)
    assert call(pkg, ctx, rows=0) == 0                                        # OK, and nothing of the ctx was needed
    assert call(pkg, ctx, rows=0, d_out=SRC) == 0                             # in place
    assert call(pkg, ctx, rows=0, d_valid=None, d_noise_valid=None) == 0      # the two that may be NULL
    assert call(pkg, ctx, rows=0, d_noise=SRC) == 0                           # the noise may be the source where out is apart
    assert call(pkg, ctx, rows=0, noise_channels=2) == 0
    assert call(pkg, ctx, rows=0, frames=0) == -1
    assert call(pkg, ctx, rows=0, d_ratio=None) == -1
