"""alacgpu_normalize_sliding_device on the GPU: bit for bit its float32 twin (sliding.sliding_host_f32), zeros comparing equal,
and within the derived bound dY of the specification (sliding.sliding_host); then `normalize` with a SlidingMeanVar.

The harness is tests/test_normalize.py's: every call reads source lines that carry NaN behind line_len and writes into an
output prefilled with NaN between guards of 0x5A bytes; the guards, what lies behind line_len and, when not in place, the source
are checked after every call.  Shapes are chosen by code path: a line of one frame, both sides of a block of 32 and of two, both
sides of the wave-per-line threshold and of the LDS limit of csrc/alac_sliding.h (above it the line goes through the ring), with
windows shorter than, as long as and longer than a line: sums of a head only, of blocks only, of head, blocks and tail."""
import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import noise, same_bits
from test_sliding_spec import offset30

pytestmark = pytest.mark.gpu

GUARD = 64
SLACK = 5


def constant(name):
    return header_constant(name, "alac_sliding.h")


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        yield torch, ctx


def run(gpu, x, how, valid=None, slack=SLACK, in_place=False):
    """One alacgpu_normalize_sliding_device call over x [rows, lines_per_row, n], as tests/test_normalize.py's run"""
    torch, ctx = gpu
    dev = torch.device("cuda", 0)
    rows, lpr, n = x.shape
    S = n + slack
    src = np.full((rows, lpr, S), np.nan, dtype=np.float32)
    src[:, :, :n] = x
    total = rows * lpr * S
    raw = torch.full(((total + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + total]
    d_src = torch.from_numpy(src).to(dev)
    if in_place:
        out.copy_(d_src.flatten())
        d_src = out
    else:
        out.fill_(float("nan"))
    d_valid = None if valid is None else torch.tensor(list(valid), dtype=torch.int64, device=dev)
    ctx.normalize_sliding_device(d_src, out, rows, lpr, S, n, d_valid, how.window, how.min_window, how.center, how.norm_vars,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + total:]]).view(torch.uint8) == 0x5A).all()), "a guard was written"
    got = out.cpu().numpy().reshape(rows, lpr, S)
    if slack:
        assert np.isnan(got[:, :, n:]).all(), "an element behind line_len was written"
    if not in_place:
        back = d_src.cpu().numpy()
        assert np.array_equal(back[:, :, :n], x, equal_nan=True) and np.isnan(back[:, :, n:]).all(), "the source was written"
    return got[:, :, :n].copy()


def check(got, x, how, valid, tag):
    from alac.net_amd.sliding import sliding_host, sliding_host_f32

    want = sliding_host_f32(x, how, valid)
    assert same_bits(got, want), (tag, "not the twin", int(np.argmax(~((got == want) | (np.isnan(got) & np.isnan(want))))))
    y, dY = sliding_host(x, how, valid, bound=True)
    ok = np.isfinite(y)
    assert np.array_equal(np.isfinite(got), ok), (tag, "not finite where the specification is, or the reverse")
    err = np.abs(got.astype(np.float64)[ok] - y[ok])
    assert (err <= dY[ok]).all(), (tag, float((err / np.maximum(dY[ok], 1e-300)).max()))


def valid_for(n, rows, turn):
    pool = [n + 5, 1, -1, n, 0, n // 2, max(n - 1, 0), (2 * n) // 3, 2]
    return [pool[(turn + 4 * r) % len(pool)] for r in range(rows)]


def small_lengths():
    wave = constant("ALAC_SLIDING_WAVE_MAX")
    return sorted({1, 31, 32, 33, 63, 64, 65, wave - 1, wave, wave + 1, 700})


@pytest.mark.parametrize("n", small_lengths())
def test_sliding_grid(gpu, n):
    from alac.net_amd.sliding import SlidingMeanVar

    turn = n
    for window in (5, 32, 33, 300, 600):
        for center in (False, True):
            for norm_vars in (False, True):
                for min_window in (1, 100):
                    how = SlidingMeanVar(window, min(min_window, window), center, norm_vars)
                    x = (noise if turn % 2 else offset30)((3, 5, n), turn)
                    valid = valid_for(n, 3, turn) if turn % 3 else None
                    got = run(gpu, x, how, valid, in_place=turn % 4 < 2, slack=0 if turn % 5 == 0 else SLACK)
                    check(got, x, how, valid, f"n {n} {how} valid {valid} turn {turn}")
                    turn += 1


def lds_lengths():
    lds = constant("ALAC_SLIDING_LDS_MAX")
    return [lds - 1, lds, lds + 1, lds + 2100]


@pytest.mark.parametrize("n", lds_lengths())
def test_both_sides_of_the_lds_limit(gpu, n):
    """Whole in LDS up to the limit, through the ring above it (lds + 2100: three chunks into the second lap)"""
    from alac.net_amd.sliding import SlidingMeanVar

    for k, how in enumerate((SlidingMeanVar(600, 100, False, True), SlidingMeanVar(33, 1, True, False), SlidingMeanVar(300, 100, True, True))):
        x = (offset30 if k == 0 else noise)((2, 1, n), n + k)
        valid = [n + 3, n - 77] if k < 2 else [n - 1100, -1]
        ref = run(gpu, x, how, valid)
        check(ref, x, how, valid, f"n {n} {how}")
        assert same_bits(run(gpu, x, how, valid, in_place=True), ref), (n, how, "in place")


def test_in_place_rows_alone_and_strides_change_nothing(gpu):
    from alac.net_amd.sliding import SlidingMeanVar

    wave = constant("ALAC_SLIDING_WAVE_MAX")
    for k, (how, n) in enumerate(((SlidingMeanVar.xvector(), wave - 55), (SlidingMeanVar(64, 10, False, True), wave + 300),
                                  (SlidingMeanVar(), 2998))):
        x = noise((3, 4, n), 70 + k)
        valid = [n - 7, -1, n // 2]
        ref = run(gpu, x, how, valid)
        assert same_bits(run(gpu, x, how, valid, in_place=True), ref), (how, n, "in place")
        assert same_bits(run(gpu, x, how, valid, slack=0), ref), (how, n, "line_stride == line_len")
        assert same_bits(run(gpu, x, how, valid, slack=0, in_place=True), ref), (how, n, "in place, line_stride == line_len")
        for r in range(3):
            assert same_bits(run(gpu, x[r:r + 1], how, valid[r:r + 1])[0], ref[r]), (how, n, "row alone", r)


def test_what_is_not_finite_reaches_its_windows_only(gpu):
    from alac.net_amd.sliding import SlidingMeanVar, sliding_windows

    wave = constant("ALAC_SLIDING_WAVE_MAX")
    for how, n in ((SlidingMeanVar(33, 5, True, False), wave - 56), (SlidingMeanVar(40, 40, False, True), wave + 200)):
        v, at = n - 7, n // 3
        valid = [v, -1, n]
        s, e = sliding_windows(v, how)
        holds = np.zeros(n, dtype=bool)
        holds[:v] = (s <= at) & (at < e)
        assert holds.any() and not holds[:v].all()
        for bad in (np.nan, np.inf):
            x = noise((3, 2, n), 9)
            x[0, 1, at] = bad
            x[0, 0, v] = np.nan                # at v
            x[0, 0, n - 1] = np.inf            # behind v
            x[1] = np.nan                      # a length of -1: nothing of the row is read
            for in_place in (False, True):
                got = run(gpu, x, how, valid, in_place=in_place)
                check(got, x, how, valid, f"{how} {bad}")
                assert np.array_equal(~np.isfinite(got[0, 1]), holds), (how, bad)
                assert np.isfinite(got[0, 0]).all() and (got[1] == 0).all() and np.isfinite(got[2]).all(), (how, bad)


def test_bad_arguments_are_refused_before_anything_is_enqueued(gpu):
    import ctypes as C

    import alac.net_amd as pkg

    torch, ctx = gpu
    rows, lpr, S, n = 2, 3, 40, 36
    src = torch.zeros(rows * lpr * S, device="cuda")
    out = torch.full((rows * lpr * S,), 7.0, device="cuda")
    valid = torch.zeros(rows, dtype=torch.int64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    lds, most = constant("ALAC_SLIDING_LDS_MAX"), constant("ALAC_SLIDING_RING_WINDOW_MAX")
    good = dict(src=p(src), out=p(out), rows=rows, lpr=lpr, S=S, n=n, valid=p(valid), window=5, min_window=3)
    bad = [dict(src=None), dict(out=None), dict(src=p(src, 2)), dict(out=p(out, 1)), dict(valid=p(valid, 4)), dict(lpr=0), dict(n=0),
           dict(n=S + 1), dict(window=0), dict(min_window=0), dict(window=1 << 31), dict(min_window=6), dict(out=p(src, 4)),
           dict(out=p(src, 4 * ((rows * lpr - 1) * S + n - 1))), dict(rows=1 << 31, S=1 << 20, n=300),
           dict(rows=1, lpr=1, S=lds + 1, n=lds + 1, window=most + 1, min_window=1)]
    call = lambda a: pkg.lib().alacgpu_normalize_sliding_device(ctx._ctx, a["src"], a["out"], a["rows"], a["lpr"], a["S"], a["n"], a["valid"],
                                                                a["window"], a["min_window"], 0, 1, None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "rows": 0}) == 0 and call({**good, "valid": None, "out": p(src)}) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_the_public_call(gpu):
    import alac.net_amd as pkg

    torch, _ = gpu
    x = offset30((3, 2, 30, 298), 4)
    d = torch.from_numpy(x).cuda()
    lengths = [298, 123, -1]
    for how in (pkg.SlidingMeanVar.xvector(), pkg.SlidingMeanVar(norm_vars=True)):
        want = pkg.normalize_host_f32(x, how, lengths)
        got = pkg.normalize(d, how, lengths)
        assert got.shape == d.shape and got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(x))
        assert same_bits(got.cpu().numpy(), want), how
        assert torch.equal(pkg.normalize(d, how, torch.tensor(lengths, device="cuda")), got)
        e = d.clone()
        assert pkg.normalize(e, how, lengths, out=e) is e and torch.equal(e, got)
        assert same_bits(pkg.normalize(d[:, 0].contiguous(), how, lengths).cpu().numpy(), want[:, 0])          # [B, lines, n]
    # the slice [..., :297]: the last column is neither read nor written
    z = x.copy()
    z[..., 297] = np.nan
    dz = torch.from_numpy(z).cuda()
    how = pkg.SlidingMeanVar.xvector()
    want = pkg.normalize_host_f32(np.ascontiguousarray(x[..., :297]), how, [297, 123, -1])
    assert pkg.normalize(dz[..., :-1], how, [297, 123, -1], out=dz[..., :-1]).data_ptr() == dz.data_ptr()
    back = dz.cpu().numpy()
    assert same_bits(back[..., :297], want) and np.isnan(back[..., 297]).all()
    assert pkg.normalize(d[:0], how).shape == (0, 2, 30, 298)
    lds = constant("ALAC_SLIDING_LDS_MAX")
    for args in ((d.cpu(), how), (d.double(), how), (d[..., ::2], how), (d, how, [1, 2]),
                 (torch.zeros(1, lds + 1, device="cuda"), pkg.SlidingMeanVar(constant("ALAC_SLIDING_RING_WINDOW_MAX") + 1))):
        with pytest.raises(ValueError):
            pkg.normalize(*args)
