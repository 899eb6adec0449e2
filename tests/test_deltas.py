"""alacgpu_deltas_device on the GPU against its float32 twin (deltas.deltas_host_f32) bit for bit -- there is no transcendental
in it, so the twin is exact -- with NaNs behind every line of the input and the output prefilled with NaN between guards of
0x5A bytes, as tests/test_fbank.py does it.  The kernel's tile is 64 frames of 4 lines."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
TILE = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    src = open(os.path.join(ROOT, "alac.net_amd", "csrc", "alac_deltas.h")).read()
    m = re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)u\s*;", src)
    assert m, f"alac_deltas.h does not define {name}"
    return int(m.group(1))


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        yield torch, pkg, ctx


def run_kernel(torch, ctx, x, spec, lengths=None, slack=5, out_slack=None):
    """The call over x [B, C, F, T] (numpy float32), stored with `slack` NaNs behind every line, into an output with `out_slack`
    elements (default: `slack` too) behind every line, prefilled with NaN, between guards; returns (out [B, C, (order + 1) F, T],
    what lies behind the lines of the output is still NaN and the guards are intact)"""
    B, C_, F, T = x.shape
    out_slack = slack if out_slack is None else out_slack
    src = np.full((B, C_, F, T + slack), np.nan, dtype=np.float32)
    src[..., :T] = x
    lines = B * C_ * (spec.order + 1) * F
    n = lines * (T + out_slack)
    raw = torch.full(((n + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device="cuda").view(torch.float32)
    raw[GUARD:GUARD + n].fill_(float("nan"))
    d_len = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
    ctx.deltas_device(torch.from_numpy(src).cuda(), raw[GUARD:], B, C_, F, T + slack, T + out_slack, T, d_len, spec.order, spec.window,
                      spec.device_scales(torch.device("cuda", 0)), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = raw[GUARD:GUARD + n].cpu().numpy().reshape(B, C_, (spec.order + 1) * F, T + out_slack)
    intact = bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all()) and bool(np.isnan(out[..., T:]).all())
    return out[..., :T], intact


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("order,window", [(1, 2), (2, 2), (3, 1), (2, 4), (3, 4), (1, 1), (1, 4), (3, 2)])
def test_kernel_equals_its_twin(gpu, order, window):
    """(3, 4) is ALAC_DELTAS_MAX_HALO, which sizes the kernel's LDS array.  (3, 2, 5, 70) and (2, 2, 3, TILE + 12) have rows
    and channels above one together, so a line's row is line / (C F) and nothing simpler; their lengths differ by row."""
    torch, pkg, ctx = gpu
    assert (header_constant("ALAC_DELTAS_MAX_ORDER"), header_constant("ALAC_DELTAS_MAX_WINDOW")) == (3, 4)
    assert TILE == header_constant("ALAC_DELTAS_TILE")
    spec = pkg.Deltas(order, window)
    rng = np.random.default_rng(10 * order + window)
    halo = order * window
    shapes = ((2, 1, 13, 198), (1, 2, 5, 33), (3, 2, 5, 70), (2, 2, 3, TILE + 12))
    for shape in shapes + tuple((3, 1, 2, T) for T in (1, 2, 4, 5, 9, TILE + 1)):
        x = (rng.standard_normal(shape) * 10).astype(np.float32)
        B, T = shape[0], shape[3]
        got, intact = run_kernel(torch, ctx, x, spec)
        assert intact and same_bits(got, pkg.deltas_host_f32(x, spec)), (shape, "whole lines")
        # lengths: T itself, 1, 0, -1, above T, and a value in the last halo of a tile
        for lens in ([T, 1, 0], [-1, T + 3, max(T - 1, 1)], [min(T, max(TILE - halo + 1, 1)), min(T, TILE), min(T, 2)]):
            lens = lens[:B]
            got, intact = run_kernel(torch, ctx, x, spec, lens)
            assert intact and same_bits(got, pkg.deltas_host_f32(x, spec, lens)), (shape, lens)


def test_source_and_output_strides_differ(gpu):
    """src_stride above out_stride and below it, at the widest filter and with a length per row: two tiles of two rows of
    two channels"""
    torch, pkg, ctx = gpu
    spec = pkg.Deltas(3, 4)
    x = (np.random.default_rng(34).standard_normal((2, 2, 3, TILE + 12)) * 10).astype(np.float32)
    for slack, out_slack in ((9, 2), (0, 7), (3, 0)):
        for lens in (None, [TILE - 3, TILE + 12], [TILE, 1]):
            got, intact = run_kernel(torch, ctx, x, spec, lens, slack=slack, out_slack=out_slack)
            assert intact and same_bits(got, pkg.deltas_host_f32(x, spec, lens)), (slack, out_slack, lens)


def test_a_nan_behind_len_stays_there(gpu):
    torch, pkg, ctx = gpu
    spec = pkg.Deltas()
    x = np.random.default_rng(3).standard_normal((2, 1, 7, 150)).astype(np.float32)
    lens = [100, 61]
    y = x.copy()
    y[0, :, :, 100:] = np.nan
    y[1, :, :, 61:] = np.inf
    clean, _ = run_kernel(torch, ctx, x, spec, lens)
    dirty, intact = run_kernel(torch, ctx, y, spec, lens)
    assert intact and same_bits(dirty[:, :, 7:], clean[:, :, 7:]) and np.isfinite(dirty[:, :, 7:]).all()
    assert same_bits(dirty[:, :, :7], y) and (dirty[0, :, 7:, 100:] == 0).all() and (dirty[1, :, 7:, 61:] == 0).all()
    # a row outside the corpus (-1): static as it is, deltas zero
    got, intact = run_kernel(torch, ctx, x, spec, [-1, 150])
    assert intact and same_bits(got[0, :, :7], x[0]) and (got[0, :, 7:] == 0).all() and got[1, :, 7:].any()


def test_add_deltas(gpu):
    torch, pkg, ctx = gpu
    spec = pkg.Deltas()
    x = np.random.default_rng(4).standard_normal((3, 2, 13, 70)).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    want = pkg.deltas_host_f32(x, spec, [70, 30, -1])
    for lens in ([70, 30, -1], torch.tensor([70, 30, -1], device="cuda"), np.array([70, 30, -1])):
        got = pkg.add_deltas(d_x, spec, lens)
        assert got.shape == (3, 2, 39, 70) and got.dtype == torch.float32 and same_bits(got.cpu().numpy(), want)
    assert same_bits(pkg.add_deltas(d_x, spec).cpu().numpy(), pkg.deltas_host_f32(x, spec))
    # the slice [..., :T] of a contiguous tensor on both sides, and out=
    wide = torch.full((3, 2, 13, 80), float("nan"), device="cuda")
    wide[..., :70] = d_x
    out = torch.full((3, 2, 39, 90), float("nan"), device="cuda")
    got = pkg.add_deltas(wide[..., :70], spec, [70, 30, -1], out=out[..., :70])
    assert got.data_ptr() == out.data_ptr() and same_bits(out[..., :70].cpu().numpy(), want) and torch.isnan(out[..., 70:]).all()
    assert pkg.add_deltas(d_x[:0], spec).shape == (0, 2, 39, 70) and pkg.add_deltas(d_x[..., :0], spec).shape == (3, 2, 39, 0)
    for bad in (lambda: pkg.add_deltas(d_x, spec, out=torch.empty(3, 2, 26, 70, device="cuda")),
                lambda: pkg.add_deltas(d_x, spec, out=torch.empty(3, 2, 39, 70, device="cuda", dtype=torch.float64)),
                lambda: pkg.add_deltas(d_x, spec, out=torch.empty(3, 2, 39, 70)),
                lambda: pkg.add_deltas(d_x, spec, out=d_x), lambda: pkg.add_deltas(d_x, spec, out=out[..., ::2][..., :35]),
                lambda: pkg.add_deltas(d_x.cpu(), spec), lambda: pkg.add_deltas(d_x[0], spec), lambda: pkg.add_deltas(d_x.double(), spec),
                lambda: pkg.add_deltas(d_x, 2), lambda: pkg.add_deltas(d_x, spec, [70, 30]), lambda: pkg.add_deltas(d_x, spec, [1.0, 2.0, 3.0]),
                lambda: pkg.add_deltas(d_x.transpose(2, 3), spec)):
        with pytest.raises(ValueError):
            bad()


def test_bad_arguments_return_before_any_enqueue(gpu):
    torch, pkg, ctx = gpu
    spec = pkg.Deltas()
    dev = torch.device("cuda", 0)
    F, T = 5, 20
    src = torch.zeros(F * T + 1, dtype=torch.float32, device=dev)
    out = torch.full((3 * F * T + 1,), 7.0, dtype=torch.float32, device=dev)
    lens = torch.tensor([T], dtype=torch.int64, device=dev)
    scales = spec.device_scales(dev)
    p = lambda t, off=0: t.data_ptr() + off
    good = dict(src=p(src), out=p(out), rows=1, channels=1, n_feats=F, src_stride=T, out_stride=T, line_len=T, lengths=p(lens), order=2,
                window=2, scales=p(scales))
    bad = [dict(src=None), dict(out=None), dict(scales=None), dict(src=p(src, 2)), dict(out=p(out, 1)), dict(scales=p(scales, 2)),
           dict(lengths=p(lens, 4)), dict(channels=0), dict(n_feats=0), dict(line_len=0), dict(line_len=T + 1), dict(src_stride=T - 1),
           dict(out_stride=T - 1), dict(order=0), dict(order=4), dict(window=0), dict(window=5), dict(channels=1 << 16, n_feats=1 << 15),
           dict(out=p(src)), dict(out=p(src, 4 * (F * T - 1))), dict(src=p(out, 4 * (3 * F * T - 1))),
           dict(rows=1 << 31, channels=2, src_stride=1 << 20, out_stride=1 << 20)]                   # 2^31 workgroups and more
    call = lambda a: pkg.lib().alacgpu_deltas_device(ctx._ctx, a["src"], a["out"], a["rows"], a["channels"], a["n_feats"], a["src_stride"],
                                                     a["out_stride"], a["line_len"], a["lengths"], a["order"], a["window"], a["scales"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    assert pkg.lib().alacgpu_deltas_device(None, *[good[k] for k in good], None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "rows": 0}) == 0                      # nothing happens
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "lengths": None}) == 0 and call(good) == 0
    torch.cuda.synchronize()
    assert (out[:3 * F * T] == 0.0).all() and out[3 * F * T] == 7.0
