"""alacgpu_level_device on the GPU against alac.net_amd/level.py: the kernel is its twin bit for bit -- the output, g, E and P -- and
within 2^-24 |s| + 2^-24 max |s| of the specification's s, at 8000 Hz (hops of 800) and 11025 Hz (hops of 1103, so chunks straddle
hops), one and two channels, the lengths around four hops and around a tile, in all three modes with max_peak and clamp;
contiguous rows and slices with aligned and odd strides and an odd base with the same bits; in place against out of place;
sentinels behind the lengths and in the rows that are not written; NaNs; no rows; the C ABI's refusals one by one."""
import sys

import numpy as np
import pytest

from test_level_spec import RATES, T, U32, lengths_of, reference, rows, specs

pytestmark = pytest.mark.gpu
SENT = 1234.5


@pytest.fixture(scope="module")
def env():
    import torch

    import alac.net_amd as pkg

    return torch, pkg, sys.modules["alac.net_amd.level"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same(a, b):
    """Bit for bit, but any NaN for any NaN (which one it is is not specified)"""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def layouts(torch, x):
    """x [B, C, T] on the device as a contiguous tensor, as slices of wider ones with an aligned and an odd stride, and at a
    base 4 bytes off 16"""
    B, C, n = x.shape
    yield "contiguous", torch.from_numpy(x).cuda()
    for name, wide in (("aligned", (n + 7) // 4 * 4), ("odd", n + 1 + n % 2)):
        w = torch.full((B, C, wide), SENT, device="cuda")
        w[..., :n] = torch.from_numpy(x).cuda()
        yield name, w[..., :n]
    flat = torch.full((B * C * n + 4,), SENT, device="cuda")
    off = flat[1:1 + B * C * n].view(B, C, n)
    off.copy_(torch.from_numpy(x))
    yield "odd-base", off


def measured(torch, pkg, lv, d, spec, rate, lens, out):
    """The entry itself, with its three outputs: (g, E, P) as numpy, out written"""
    from alac.net_amd._stageargs import _planes
    from alac.net_amd.resample import _context

    B, C, n = d.shape
    mode, hop = lv._checked(spec, rate, C)
    q = lv._kweight_device(float(rate), str(d.device)) if mode == lv.LUFS else None
    res = [torch.full((B,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
    valid = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int64)).cuda()
    _context(0).level_device(d, out, B, C, _planes("x", d), n, valid, mode, hop, q, spec.linear, spec.max_peak or 0.0, spec.clamp, *res,
                             stream=torch.cuda.current_stream().cuda_stream)
    return [r.cpu().numpy() for r in res]


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", ["peak", "rms", "lufs", "lufs-max-peak", "rms-clamp", "peak-max-peak"])
def test_the_kernel_is_its_twin_and_within_the_bound(env, rate, name):
    torch, pkg, lv = env
    x, lens = rows(rate)
    spec = specs()[name]
    (s, g, E, P), (twin, gt, Et, Pt) = reference(rate, name)
    v = np.clip(lens, 0, T)
    written = (gt != 1.0) | (spec.clamp & (Et != 0.0) & (v > 0))
    first = None
    for lay, d in layouts(torch, np.array(x)):
        # out of place into sentinels: the frames at or behind v and the rows that are not written keep them
        out = torch.empty_strided(d.shape, d.stride(), dtype=d.dtype, device="cuda").fill_(SENT)        # (d's own layout)
        got_g, got_E, got_P = measured(torch, pkg, lv, d, spec, rate, lens, out)
        got = out.cpu().numpy()
        assert same(got_g, gt) and same(got_E, Et) and same(got_P, Pt), (lay, got_g, gt)
        for b in range(len(lens)):
            if written[b]:
                assert same(got[b, :, :v[b]], twin[b, :, :v[b]]), (lay, b)
                assert (got[b, :, v[b]:] == SENT).all(), (lay, b)
            else:
                assert (got[b] == SENT).all(), (lay, b)
        # the public call: a copy of x with the rows levelled, and in place the same bits
        y = pkg.level(d, spec, rate, lens)
        assert same(y.cpu().numpy(), twin), lay
        first = y if first is None else first
        assert torch.equal(y.view(torch.int32), first.view(torch.int32)), lay
        e = d.clone() if lay == "contiguous" else d
        assert pkg.level(e, spec, rate, lens, out=e) is e and torch.equal(e.view(torch.int32), first.view(torch.int32)), lay
        if lay in ("aligned", "odd"):
            assert bool((d._base[..., T:] == SENT).all()), lay
    err = np.abs(first.cpu().numpy().astype(np.float64) - s)
    peak = np.abs(s).max(axis=(1, 2), keepdims=True)
    print(f"{name} at {rate} Hz: kernel against the specification at most {float((err / np.maximum(peak, 1e-300)).max()):.3e} of the row's peak")
    assert np.all(err <= U32 * np.abs(s) + U32 * peak)


@pytest.mark.parametrize("rate", RATES)
def test_one_channel(env, rate):
    torch, pkg, lv = env
    x, lens = rows(rate)
    x1 = np.ascontiguousarray(x[:, 1:])
    for name in ("peak", "rms", "lufs", "lufs-max-peak"):
        spec = specs()[name]
        twin, gt, Et, Pt = pkg.level_host_twin(x1, spec, rate, lens, details=True)
        d = torch.from_numpy(x1).cuda()
        out = d.clone()
        got = measured(torch, pkg, lv, d, spec, rate, lens, out)
        assert same(out.cpu().numpy(), twin) and same(got[0], gt) and same(got[1], Et) and same(got[2], Pt), name


def test_loudness_and_no_lengths(env):
    torch, pkg, lv = env
    for rate in RATES:
        x, lens = rows(rate)
        d = torch.from_numpy(np.array(x)).cuda()
        keep = d.clone()
        got = pkg.loudness(d, rate, lens).cpu().numpy()
        E = pkg.level_host_twin(x, lv.Level.lufs(), rate, lens, details=True)[2]
        assert torch.equal(d, keep) and got.dtype == np.float64
        assert np.array_equal(np.isinf(got), E == 0.0) and (got[E == 0.0] == -np.inf).all()
        want = -0.691 + 10.0 * np.log10(E[E != 0.0])
        assert np.abs(got[E != 0.0] - want).max() <= 1e-12
        full = pkg.level(d, lv.Level.lufs(-30.0), rate)
        assert same(full.cpu().numpy(), pkg.level_host_twin(x, lv.Level.lufs(-30.0), rate))
    assert pkg.loudness(torch.zeros(0, 2, 100, device="cuda"), 8000).shape == (0,)


def test_a_nan_stays_in_its_row_and_behind_v_is_never_read(env):
    torch, pkg, lv = env
    rate = 11025
    x, lens = rows(rate)
    bad = np.array(x)
    bad[11, 1, 5000] = np.nan            # below v of the last row
    bad[10, 0, 8192] = np.nan            # at v of row 10: never read
    bad[9, 0, 6000] = np.inf             # behind v of row 9
    for name in ("peak", "rms-clamp", "lufs", "lufs-max-peak"):
        spec = specs()[name]
        clean = reference(rate, name)[1]
        d = torch.from_numpy(bad).cuda()
        got_g, got_E, got_P = measured(torch, pkg, lv, d, spec, rate, lens, d)
        got = d.cpu().numpy()
        twin, gt, Et, Pt = pkg.level_host_twin(bad, spec, rate, lens, details=True)
        assert same(got, twin) and same(got_g, gt) and same(got_E, Et) and same(got_P, Pt), name
        assert np.isnan(got_P[11]) and np.isnan(got[11, 1, 5000])
        assert same(got[:9], clean[0][:9]) and same(got[9, :, :4097], clean[0][9, :, :4097]) and same(got_g[:11], clean[1][:11]), name
        assert same(got[10, :, :8192], clean[0][10, :, :8192]) and np.isnan(got[10, 0, 8192]) and got[9, 0, 6000] == np.inf, name
        if not name.startswith("lufs"):
            assert np.isnan(got_g[11]) and np.isnan(got[11, :, :T]).all()


def test_what_level_refuses_and_no_rows(env):
    torch, pkg, lv = env
    L = pkg.Level
    d = torch.zeros(2, 2, 4000, device="cuda")
    for args in ((d.cpu(), L.peak()), (d.double(), L.peak()), (d[0], L.peak()), (d[..., ::2], L.peak()), (d, "peak"), (d, L.lufs()),
                 (d, L.lufs(), 150), (d, L.lufs(), 3000), (torch.zeros(1, 6, 4000, device="cuda"), L.lufs(), 8000), (d, L.rms(), 8000, [1, 2, 3]),
                 (d, L.rms(), 8000, [1.0, 2.0])):
        with pytest.raises(ValueError):
            pkg.level(*args)
    for out in (d[..., :-1], d.double(), d.cpu(), torch.empty(2, 2, 4001, device="cuda")[..., :4000]):
        with pytest.raises(ValueError):
            pkg.level(d, L.rms(), 8000, out=out)
    with pytest.raises(ValueError):
        pkg.loudness(d, 100)
    assert pkg.level(torch.zeros(0, 2, 8, device="cuda"), L.lufs(), 8000).shape == (0, 2, 8)
    assert bool((pkg.level(d, L.lufs(), 8000) == 0).all())               # silence stays silence


def test_the_c_abi_refuses_item_by_item(env):
    torch, pkg, lv = env
    rows_, C, stride, n = 3, 2, 80, 72
    src = torch.zeros(rows_ * C * stride + 8, device="cuda")
    out = torch.full((rows_ * C * stride + 8,), 7.0, device="cuda")
    q = torch.from_numpy(lv.kweight(8000)).cuda()
    valid = torch.full((rows_ + 1,), n, dtype=torch.int64, device="cuda")
    res = [torch.full((rows_ + 1,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
    base = dict(d_src=src.data_ptr(), d_out=out.data_ptr(), rows=rows_, channels=C, stride=stride, frames=n, d_valid=valid.data_ptr(),
                mode=2, hop=16, d_kweight=q.data_ptr(), target=0.01, max_peak=0.0, clamp=0, d_gain=res[0].data_ptr(),
                d_energy=res[1].data_ptr(), d_peak=res[2].data_ptr(), stream=None)
    extent = 4 * ((rows_ * C - 1) * stride + n)
    cases = [dict(d_src=None), dict(d_kweight=None), dict(d_out=None, d_gain=None, d_energy=None, d_peak=None),
             dict(d_src=base["d_src"] + 2), dict(d_out=base["d_out"] + 2), dict(d_valid=base["d_valid"] + 4),
             dict(d_kweight=base["d_kweight"] + 4), dict(d_gain=base["d_gain"] + 4), dict(d_energy=base["d_energy"] + 4),
             dict(d_peak=base["d_peak"] + 4), dict(mode=3), dict(channels=0), dict(channels=6, rows=1), dict(hop=15), dict(frames=0),
             dict(frames=stride + 1), dict(stride=n - 1), dict(target=0.0), dict(target=float("nan")), dict(target=float("inf")),
             dict(max_peak=float("nan")), dict(d_out=base["d_src"] + 4), dict(d_out=base["d_src"] + extent - 4),
             dict(d_gain=base["d_out"] + 8), dict(d_energy=base["d_out"] + extent - 8), dict(d_peak=base["d_src"] + 16),
             dict(d_kweight=base["d_out"] + 16), dict(stride=1 << 58),
             dict(d_out=base["d_src"], rows=1 << 31, channels=1, stride=1, frames=1, mode=0, d_kweight=None, d_gain=base["d_src"] + (1 << 44),
                  d_energy=None, d_peak=None)]
    fn = pkg.lib().alacgpu_level_device
    with pkg.AlacGpuContext([(512, 16, 40, 10, 14, 2)]) as ctx:
        for change in cases:
            assert fn(ctx._ctx, *dict(base, **change).values()) == -1, change
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((src == 0).all()) and all(bool((r == -7.0).all()) for r in res)
        # ... and the same arguments unchanged are a call, as is one of no rows, of no lengths, of no outputs and of no d_out;
        # the other modes take more than 5 channels, any hop and no d_kweight
        assert fn(ctx._ctx, *dict(base, rows=0).values()) == 0
        assert fn(ctx._ctx, *dict(base, d_valid=None, d_gain=None, d_energy=None, d_peak=None).values()) == 0
        assert fn(ctx._ctx, *dict(base, d_out=None).values()) == 0
        assert fn(ctx._ctx, *dict(base, mode=1, channels=6, rows=1, hop=0, d_kweight=None).values()) == 0
        assert fn(ctx._ctx, *base.values()) == 0
        torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # silence: nothing to measure, nothing written
    assert [r[:rows_].tolist() for r in res] == [[1.0] * rows_, [0.0] * rows_, [0.0] * rows_] and all(float(r[rows_]) == -7.0 for r in res)
