"""The host side of the normalisations (alac.net_amd/normalize.py): the float64 specification against numpy and torch, the
float32 twin against the derived bound dY, a mutant twin that the bound's criterion must see, and the arguments of the spec
classes and of the two entry points.  CPU only.

The twin criterion: on an input, r = max |evaluation - specification| / dY.  dY bounds every float32 evaluation in any
order, so the twin has r <= 1; the tests on the GPU hold the kernel to r_gpu <= 4 r_twin (tests/test_features.py's
check_power and its factor).  The mutant shows that criterion has teeth: E[x^2] - mean^2 in float32 on a signal with a DC
offset of 0.9 and noise of 1e-3 loses the variance's leading digits, and its r is far more than 4 times the twin's."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def noise(shape, seed):
    """full-scale noise, uniform in -1 .. 1"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def dc(shape, seed):
    """0.9 + 1e-3 * noise: the input on which E[x^2] - mean^2 fails in float32"""
    return (0.9 + 1e-3 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def same_bits(a, b):
    """bit for bit, where zeros compare equal and a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_whisper_is_torch_maximum_and_affine_bit_for_bit():
    import torch

    from alac.net_amd.normalize import TopDb, normalize_host_f32

    assert TopDb.whisper() == TopDb(8.0, 0.25, 1.0)
    x = np.random.default_rng(1).uniform(-10.0, 2.0, (5, 2, 80, 37)).astype(np.float32)
    x[0, 0, 3, 5] = 2.0                       # one row whose maximum is the top of the range
    x[1] = np.minimum(x[1], -9.0)             # ... and one that lies below -8 throughout
    got = normalize_host_f32(x, TopDb.whisper())
    for b in range(x.shape[0]):
        t = torch.from_numpy(x[b])
        want = (torch.maximum(t, t.max() - 8.0) + 4.0) / 4.0
        assert want.dtype == torch.float32
        assert same_bits(got[b], want.numpy()), b
    # per channel: every x[b, c] against its own maximum
    got = normalize_host_f32(x, TopDb(8.0, 0.25, 1.0, per_channel=True))
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            t = torch.from_numpy(x[b, c])
            assert same_bits(got[b, c], ((torch.maximum(t, t.max() - 8.0) + 4.0) / 4.0).numpy()), (b, c)


def test_decibels_relative_in_numpy_float32():
    from alac.net_amd.normalize import TopDb, normalize_host, normalize_host_f32

    f32 = np.float32
    assert TopDb.decibels(80.0, relative=True) == TopDb(8.0, 10.0, 0.0, True)
    assert TopDb.decibels() == TopDb(8.0, 10.0, 0.0, False)
    x = np.random.default_rng(2).uniform(-10.0, 2.0, (4, 1, 16, 51)).astype(np.float32)
    how = TopDb.decibels(80.0, relative=True)
    got = normalize_host_f32(x, how)
    for b in range(4):
        mx = x[b].max()
        want = (f32(10) * (np.maximum(x[b], (mx - f32(8)).astype(f32)) - mx).astype(f32)).astype(f32)
        assert same_bits(got[b], want), b
        assert got[b].max() == 0.0 and got[b].min() >= -80.0
    # the twin inside the specification's own bound, and the specification what the formula says in float64
    y, dY = normalize_host(x, how, bound=True)
    assert (np.abs(got.astype(np.float64) - y) <= dY).all()
    x64 = x.astype(np.float64)
    mx = x64.max(axis=(1, 2, 3), keepdims=True)
    assert np.array_equal(y, 10.0 * (np.maximum(x64, mx - 8.0) - mx))
    # a NaN: its row is NaN throughout, every other row what it was
    z = x.copy()
    z[2, 0, 7, 7] = np.nan
    for fn in (normalize_host, normalize_host_f32):
        a, b = fn(x, how), fn(z, how)
        assert np.isnan(b[2]).all() and np.array_equal(np.delete(a, 2, 0), np.delete(b, 2, 0))


def test_meanvar_specification_against_numpy():
    from alac.net_amd.normalize import MeanVar, normalize_host

    x = noise((6, 2, 3, 50), 3) * 3.0 + 0.5
    lengths = [50, 17, 1, 0, -1, 55]
    for eps in (0.0, 1e-5):
        y = normalize_host(x, MeanVar(eps=eps), lengths)
        assert y.dtype == np.float64 and y.shape == x.shape
        for b, L in enumerate(lengths):
            v = min(max(L, 0), 50)                                   # -1 counts as 0, 55 as the line's 50
            assert (y[b, ..., v:] == 0).all()
            for c in range(2):
                for m in range(3):
                    seg = x[b, c, m, :v].astype(np.float64)
                    if v:
                        with np.errstate(invalid="ignore"):
                            want = (seg - seg.mean()) / np.sqrt(seg.var() + float(np.float32(eps)))
                        if v == 1 and eps == 0.0:
                            assert np.isnan(y[b, c, m, 0])            # a constant line without eps: 0 / 0
                        else:
                            np.testing.assert_allclose(y[b, c, m, :v], want, rtol=1e-12, atol=1e-12)
    # without lengths: whole lines
    np.testing.assert_allclose(normalize_host(x, MeanVar()), normalize_host(x, MeanVar(), [50] * 6), rtol=0, atol=0)
    # centre and scale alone
    seg = x[0, 1, 2].astype(np.float64)
    np.testing.assert_allclose(normalize_host(x, MeanVar(scale=False))[0, 1, 2], seg - seg.mean(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(normalize_host(x, MeanVar(centre=False))[0, 1, 2], seg / np.sqrt(seg.var()), rtol=1e-12, atol=1e-12)
    # a constant line: NaN without eps, zeros with
    k = np.full((1, 1, 9), 0.25, dtype=np.float32)
    from alac.net_amd.normalize import normalize_host_f32
    for fn in (normalize_host, normalize_host_f32):
        assert np.isnan(fn(k, MeanVar())).all()
        assert (fn(k, MeanVar(eps=1e-5)) == 0).all()
        assert (fn(k, MeanVar(), [-1]) == 0).all()
    # a NaN stays in its line; one at or behind v changes nothing
    z = x.copy()
    z[1, 0, 1, 16] = np.nan
    z[1, 1, 2, 17] = np.nan          # (lengths[1] = 17: index 17 is behind v)
    for fn in (normalize_host, normalize_host_f32):
        a, b = fn(x, MeanVar(), lengths), fn(z, MeanVar(), lengths)
        assert np.isnan(b[1, 0, 1, :17]).all() and (b[1, 0, 1, 17:] == 0).all()
        b[1, 0, 1] = a[1, 0, 1]
        assert same_bits(a, b)


TWIN_INPUTS = [("noise 201", lambda: noise((3, 2, 5, 201), 4), [201, 77, 150]),
               ("dc 201", lambda: dc((3, 2, 5, 201), 5), [201, 77, 150]),
               ("noise 1500", lambda: noise((2, 1, 3, 1500), 6), [1500, 1031]),
               ("noise 64", lambda: noise((2, 4, 64), 7), None)]


def ratio(y32, y, dY):
    live = dY > 0
    return float(np.max(np.abs(y32.astype(np.float64) - y)[live] / dY[live])) if live.any() else 0.0


@pytest.mark.parametrize("tag,make,lengths", TWIN_INPUTS, ids=[t[0] for t in TWIN_INPUTS])
def test_the_twin_lies_inside_the_bound_and_the_bound_is_not_vacuous(tag, make, lengths):
    from alac.net_amd.normalize import MeanVar, normalize_host, normalize_host_f32

    x = make()
    for how in (MeanVar(), MeanVar(eps=1e-5), MeanVar(scale=False), MeanVar(centre=False)):
        y, dY = normalize_host(x, how, lengths, bound=True)
        y32 = normalize_host_f32(x, how, lengths)
        assert y32.dtype == np.float32 and np.isfinite(y32).all() and np.isfinite(dY).all()
        err = np.abs(y32.astype(np.float64) - y)
        print(f"{tag} {how}: max |y| {np.abs(y).max():.3f}, max err {err.max():.3e}, r {ratio(y32, y, dY):.4f}, "
              f"dY <= 0.1 in {np.mean(dY <= 0.1):.3f}, max dY {dY.max():.3e}")
        assert (err <= dY).all(), (tag, how, int(np.argmax(err - dY)))
        # not vacuous: a result of size 1 is pinned to 0.1; with centre off a result is x / s, hundreds on the DC input,
        # and is pinned to a tenth of its own size
        narrow = dY <= 0.1 * (1.0 if how.centre else np.maximum(np.abs(y), 1.0))
        assert np.mean(narrow) >= 0.9, (tag, how)
        v = np.clip(np.asarray(lengths if lengths is not None else [x.shape[-1]] * x.shape[0]), 0, x.shape[-1])
        for b, k in enumerate(v):
            assert (y32[b, ..., k:] == 0).all() and (dY[b, ..., k:] == 0).all()


def mutant_f32(x):
    """A twin that takes the variance as E[x^2] - mean^2, each step in float32"""
    f32 = np.float32
    n = f32(x.shape[-1])
    mean = (x.sum(axis=-1, keepdims=True, dtype=f32) / n).astype(f32)
    ex2 = ((x * x).astype(f32).sum(axis=-1, keepdims=True, dtype=f32) / n).astype(f32)
    var = (ex2 - (mean * mean).astype(f32)).astype(f32)
    with np.errstate(all="ignore"):
        return ((x - mean).astype(f32) / np.sqrt(np.maximum(var, f32(0))).astype(f32)).astype(f32)


def test_the_criterion_sees_a_one_pass_variance():
    from alac.net_amd.normalize import MeanVar, normalize_host, normalize_host_f32

    x = dc((3, 2, 5, 201), 5)
    y, dY = normalize_host(x, MeanVar(), bound=True)
    r_twin = ratio(normalize_host_f32(x, MeanVar()), y, dY)
    m = mutant_f32(x)
    err = np.abs(m.astype(np.float64) - y)
    r_mutant = float(np.max(np.where(np.isfinite(err), err, np.inf) / dY))
    print(f"dc input: r_twin {r_twin:.4f}, r_mutant {r_mutant:.4f}, ratio {r_mutant / r_twin:.1f}")
    assert 0 < r_twin <= 1
    assert r_mutant > 4 * r_twin


def test_spec_classes_refuse_what_the_library_refuses():
    from alac.net_amd.normalize import MeanVar, TopDb, normalize_host, normalize_host_f32

    assert MeanVar() == MeanVar(True, True, 0.0) and MeanVar().eps == 0.0 and hash(MeanVar()) == hash(MeanVar())
    assert TopDb() == TopDb(8.0, 1.0, 0.0, False, False)
    for bad in (dict(eps=-1e-9), dict(eps=INF), dict(eps=NAN), dict(eps=1e39), dict(eps="1"), dict(centre=False, scale=False),
                dict(centre=1), dict(scale=None)):
        with pytest.raises(ValueError):
            MeanVar(**bad)
    for bad in (dict(top=-0.5), dict(top=INF), dict(top=NAN), dict(top=1e39), dict(scale=INF), dict(scale=NAN), dict(scale=-1e39),
                dict(offset=INF), dict(offset=NAN), dict(offset="0"), dict(relative=1), dict(per_channel=0)):
        with pytest.raises(ValueError):
            TopDb(**bad)
    for bad in (-1.0, INF, NAN):
        with pytest.raises(ValueError):
            TopDb.decibels(bad)
    assert TopDb(top=0.0).top == 0.0 and TopDb(scale=-2.0).scale == -2.0
    for spec in (MeanVar(), TopDb()):
        with pytest.raises(AttributeError):
            spec.eps = 1.0
        with pytest.raises(AttributeError):
            del spec.relative
    x = np.zeros((2, 3, 8), dtype=np.float32)
    for fn in (normalize_host, normalize_host_f32):
        for args in ((x.astype(np.float64), MeanVar()), (x, "meanvar"), (x[0, 0], MeanVar()), (x[:, 0], TopDb(per_channel=True)),
                     (x, MeanVar(), [1, 2, 3]), (x, MeanVar(), [1.0, 2.0])):
            with pytest.raises(ValueError):
                fn(*args)


def header_args(name):
    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"include/alacgpu.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


def test_the_entry_points_are_declared_bound_and_exported():
    import alac.net_amd as pkg

    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    for name in ("alacgpu_normalize_meanvar_device", "alacgpu_normalize_top_device"):
        args = header_args(name)
        assert len(args) == len(pkg.SYMBOLS[name][1]) == 12
        assert hasattr(pkg.lib(), name)
        m = re.search(r"extern\s+int\s+" + name + r"\s*\(([^)]*)\)", cs)
        assert m, f"AlacGpuNative.cs does not declare {name}"
        assert len(m.group(1).split(",")) == 12
    assert pkg.lib().alacgpu_version() == 3
    for n in ("MeanVar", "TopDb", "normalize", "normalize_host", "normalize_host_f32"):
        assert hasattr(pkg, n)
    assert hasattr(pkg.AlacGpuContext, "normalize_meanvar_device") and hasattr(pkg.AlacGpuContext, "normalize_top_device")


# A call's arguments in the header's order.  The pointers are numbers: an argument check never follows one, and every case
# below returns from the check -- a call that passed it would use the ctx, which here is a page of zeros.
SRC, OUT, VALID = 0x10000, 0x20000, 0x30000
MEANVAR = dict(d_src=SRC, d_out=OUT, rows=2, lines_per_row=3, line_stride=16, line_len=10, d_valid=VALID, centre=1, scale=1,
               eps=0.0, stream=None)
TOP = dict(d_src=SRC, d_out=OUT, rows=2, lines_per_row=3, line_stride=16, line_len=10, top=8.0, scale=0.25, offset=1.0,
           relative=0, stream=None)
EXTENT = 4 * (5 * 16 + 10)       # bytes from the first element of the arrays above to behind their last
BOTH = [dict(d_src=None), dict(d_out=None), dict(d_src=SRC + 2), dict(d_out=OUT + 2), dict(d_out=OUT + 1),
        dict(lines_per_row=0), dict(line_len=0), dict(line_len=17), dict(line_stride=9),
        dict(d_out=SRC + 4), dict(d_out=SRC + EXTENT - 4), dict(d_src=OUT + EXTENT - 4), dict(d_out=SRC + 64),
        dict(rows=2 ** 32 - 1, lines_per_row=2 ** 32 - 1, line_stride=2 ** 40, line_len=2 ** 40)]
CASES = ([("meanvar", c) for c in BOTH] + [("top", c) for c in BOTH] +
         [("meanvar", c) for c in (dict(d_valid=VALID + 4), dict(eps=-1e-6), dict(eps=INF), dict(eps=NAN), dict(centre=0, scale=0),
                                   dict(rows=2 ** 31, lines_per_row=1, line_len=257, line_stride=257),                 # one workgroup per line
                                   dict(rows=2 ** 32 - 1, lines_per_row=4, line_len=256, line_stride=256))] +      # four lines per workgroup
         [("top", c) for c in (dict(top=-1.0), dict(top=INF), dict(top=NAN), dict(scale=INF), dict(scale=NAN), dict(offset=-INF),
                               dict(offset=NAN), dict(rows=2 ** 31, lines_per_row=1),
                               dict(rows=2 ** 30, lines_per_row=1, line_len=4097, line_stride=4097))])             # two parts per row


def call(pkg, which, ctx, **kw):
    base = dict(MEANVAR if which == "meanvar" else TOP, **kw)
    fn = getattr(pkg.lib(), f"alacgpu_normalize_{which}_device")
    return fn(ctx, *base.values())


@pytest.mark.parametrize("which,change", CASES, ids=[f"{w}-{'-'.join(c)}-{i}" for i, (w, c) in enumerate(CASES)])
def test_bad_arguments_are_refused_before_anything_is_enqueued(which, change):
    import alac.net_amd as pkg

    page = ctypes.create_string_buffer(4096)
    assert call(pkg, which, ctypes.addressof(page), **change) == -1, (which, change)


def test_a_null_ctx_is_refused_and_no_rows_are_no_work():
    import alac.net_amd as pkg

    page = ctypes.create_string_buffer(4096)
    for which in ("meanvar", "top"):
        assert call(pkg, which, None) == -1                                    # every other argument is valid
        assert call(pkg, which, None, rows=0) == -1
        assert call(pkg, which, ctypes.addressof(page), rows=0) == 0           # OK, and nothing of the ctx was needed
        assert call(pkg, which, ctypes.addressof(page), rows=0, d_out=SRC) == 0
        assert call(pkg, which, ctypes.addressof(page), rows=0, line_len=0) == -1
    assert call(pkg, "meanvar", ctypes.addressof(page), rows=0, d_valid=None) == 0
