"""alacgpu_vad_energy_device and alacgpu_select_frames_device on the GPU, bit for bit their specifications in numpy
(vad.vad_host_f32, vad.select_host), then `vad_energy` and `select_frames`.

The harness is tests/test_normalize.py's: sources with NaN slack behind every line, outputs (the decisions too) prefilled
between guards of 0x5A bytes; the guards, the slack and, when not in place, the source are checked after every call."""
import ctypes as C

import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import noise, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SLACK = 5


def constant(name):
    return header_constant(name, "alac_vad.h")


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        yield torch, ctx


def run_vad(gpu, x, vad, valid):
    """One alacgpu_vad_energy_device call over x [B, C, lines, n]: NaN slack behind every line, the decisions into uint8
    [B, n + SLACK] prefilled with 0xA5 between guards of 0x5A.  Returns the decisions [B, n]."""
    torch, ctx = gpu
    B, C_, lines, n = x.shape
    S = n + SLACK
    src = np.full((B, C_, lines, S), np.nan, dtype=np.float32)
    src[..., :n] = x
    d_src = torch.from_numpy(src).cuda()
    raw = torch.full((B * S + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    mask = raw[GUARD:GUARD + B * S]
    mask.fill_(0xA5)
    d_valid = None if valid is None else torch.tensor(list(valid), dtype=torch.int64, device="cuda")
    ctx.vad_energy_device(d_src, B, C_ * lines * S, vad.line * S, n, d_valid, vad.energy_threshold, vad.energy_mean_scale,
                          vad.frames_context, vad.proportion_threshold, mask, S, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + B * S:]]) == 0x5A).all()), "a guard was written"
    got = mask.cpu().numpy().reshape(B, S)
    assert (got[:, n:] == 0xA5).all(), "a byte behind line_len was written"
    assert np.array_equal(d_src.cpu().numpy(), src, equal_nan=True), "the source was written"
    return got[:, :n].copy()


@pytest.mark.parametrize("n", [1, 200, 256, 257, 1500])
def test_vad_is_the_twin_bit_for_bit(gpu, n):
    """Both sides of the threshold between 64 and 1024 partial sums (256 frames); [4, 1, 13, n] and [2, 2, 30, n]"""
    from alac.net_amd.vad import EnergyVad, vad_host_f32

    assert constant("ALAC_VAD_WAVE_MAX") == 256
    voiced = 0
    for shape, valid in (((4, 1, 13, n), [n, (2 * n) // 3, 0, -1]), ((2, 2, 30, n), [n + 4, max(n - 1, 1)]), ((5, 1, 13, n), None)):
        for line in (0, 3):
            for context in (0, 2):
                for thr, scale, prop in ((5.5, 0.5, 0.12), (5.0, 0.5, 0.6), (8.0, 0.0, 1.0)):
                    vad = EnergyVad(thr, scale, context, prop, line)
                    x = (8.0 + 6.0 * noise(shape, n + line + context)).astype(np.float32)
                    got = run_vad(gpu, x, vad, valid)
                    want = vad_host_f32(x, vad, valid)
                    assert np.array_equal(got, want), (shape, vad, valid)
                    voiced += int(got.sum())
    assert voiced > 0
    # NaN energies: they compare false, and make the threshold NaN unless the scale is 0
    x = (8.0 + 6.0 * noise((3, 1, 13, n), 5)).astype(np.float32)
    x[0, 0, 0, n // 2] = np.nan
    for vad in (EnergyVad(5.0, 0.5, 1, 0.6), EnergyVad(5.0, 0.0, 1, 0.6), EnergyVad(5.0, 0.5, 1, 0.0)):
        assert np.array_equal(run_vad(gpu, x, vad, None), vad_host_f32(x, vad)), vad


def run_select(gpu, x, mask, valid, in_place=False, over_valid=False, slack=SLACK):
    """One alacgpu_select_frames_device call over x [rows, lines_per_row, n] and mask [rows, n]; over_valid: the new lengths
    are written over d_valid itself.  Returns (out [rows, lines_per_row, n], new_lengths)."""
    torch, ctx = gpu
    rows, lpr, n = x.shape
    S = n + slack
    src = np.full((rows, lpr, S), np.nan, dtype=np.float32)
    src[:, :, :n] = x
    total = rows * lpr * S
    raw = torch.full(((total + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device="cuda").view(torch.float32)
    out = raw[GUARD:GUARD + total]
    d_src = torch.from_numpy(src).cuda()
    if in_place:
        out.copy_(d_src.flatten())
        d_src = out
    else:
        out.fill_(float("nan"))
    m = np.full((rows, n + 3), 1, dtype=np.uint8)                   # (ones behind line_len: never read)
    m[:, :n] = mask
    d_mask = torch.from_numpy(m).cuda()
    d_valid = None if valid is None else torch.tensor(list(valid), dtype=torch.int64, device="cuda")
    lens = torch.full((rows + 2,), -77, dtype=torch.int64, device="cuda")
    d_new = d_valid if over_valid else lens[1:rows + 1]
    ctx.select_frames_device(d_src, out, rows, lpr, S, n, d_valid, d_mask, n + 3, d_new, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + total:]]).view(torch.uint8) == 0x5A).all()), "a guard was written"
    assert lens[0] == -77 and lens[-1] == -77 and np.array_equal(d_mask.cpu().numpy(), m)
    if valid is not None and not over_valid:
        assert d_valid.tolist() == list(valid)
    got = out.cpu().numpy().reshape(rows, lpr, S)
    if slack:
        assert np.isnan(got[:, :, n:]).all(), "an element behind line_len was written"
    if not in_place:
        back = d_src.cpu().numpy()
        assert np.array_equal(back[:, :, :n], x, equal_nan=True) and np.isnan(back[:, :, n:]).all(), "the source was written"
    return got[:, :, :n].copy(), d_new.cpu().numpy()


def masks(rows, n, seed):
    """all ones, all zeros, alternating, one voiced frame at each end, then random ones"""
    m = (np.random.default_rng(seed).uniform(size=(rows, n)) < 0.6).astype(np.uint8)
    m[0] = 1
    if rows > 1:
        m[1] = 0
    if rows > 2:
        m[2] = np.arange(n) % 2
    if rows > 3:
        m[3] = 0
        m[3, 0] = m[3, n - 1] = 1
    return m


def select_lengths():
    chunk = constant("ALAC_SELECT_CHUNK")
    return [1, 2, 300, chunk - 1, chunk, chunk + 1, 2 * chunk + 77]


@pytest.mark.parametrize("n", select_lengths())
def test_select_is_the_specification_bit_for_bit(gpu, n):
    from alac.net_amd.vad import select_host

    per = constant("ALAC_SELECT_LINES")
    for lpr in (1, per, per + 3):
        x = noise((6, lpr, n), n + lpr)
        x[x == 0] = 1.0
        m = masks(6, n, n)
        for valid in (None, [n, n + 2, n, n, max(n - 3, 0), -1]):
            want, new = select_host(x, m, valid)
            if valid is None or valid[0] == n:
                assert same_bits(want[0], x[0])                   # all ones over a whole line: an exact copy
            for in_place in (False, True):
                for over_valid in ((False, True) if valid is not None else (False,)):
                    got, lens = run_select(gpu, x, m, valid, in_place, over_valid, slack=0 if n % 2 else SLACK)
                    assert same_bits(got, want), (n, lpr, valid, in_place, over_valid)
                    assert lens.tolist() == new.tolist(), (n, lpr, valid, in_place, over_valid)


def test_bad_arguments_are_refused_before_anything_is_enqueued(gpu):
    import alac.net_amd as pkg

    torch, ctx = gpu
    rows, lpr, S, n = 2, 3, 40, 36
    src = torch.zeros(rows * lpr * S, device="cuda")
    out = torch.full((rows * lpr * S,), 7.0, device="cuda")
    valid = torch.zeros(rows, dtype=torch.int64, device="cuda")
    new = torch.full((rows + 1,), 7, dtype=torch.int64, device="cuda")
    mask = torch.full((rows * S,), 7, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    nan, inf = float("nan"), float("inf")
    # the decision
    good = dict(src=p(src), rows=rows, row_stride=lpr * S, line=S, n=n, valid=p(valid), thr=5.0, scale=0.5, context=2, prop=0.6,
                mask=p(mask), mask_stride=S)
    bad = [dict(src=None), dict(mask=None), dict(src=p(src, 2)), dict(valid=p(valid, 4)), dict(n=0), dict(n=S + 1, row_stride=10 * S),
           dict(line=2 * S + 5), dict(line=lpr * S + 1), dict(thr=nan), dict(thr=inf), dict(scale=nan), dict(scale=-0.5), dict(scale=inf),
           dict(context=constant("ALAC_VAD_MAX_CONTEXT") + 1), dict(prop=-0.1), dict(prop=1.5), dict(prop=nan),
           dict(mask=C.c_void_p(src.data_ptr() + 8)), dict(rows=1 << 31, row_stride=1 << 20, n=300, mask_stride=300, line=0)]
    call = lambda a: pkg.lib().alacgpu_vad_energy_device(ctx._ctx, a["src"], a["rows"], a["row_stride"], a["line"], a["n"], a["valid"], a["thr"],
                                                         a["scale"], a["context"], a["prop"], a["mask"], a["mask_stride"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    assert call({**good, "rows": 0}) == 0
    # the selection
    good = dict(src=p(src), out=p(out), rows=rows, lpr=lpr, S=S, n=n, valid=p(valid), mask=p(mask), mask_stride=S, new=p(new))
    bad = [dict(src=None), dict(out=None), dict(mask=None), dict(new=None), dict(src=p(src, 2)), dict(out=p(out, 1)), dict(valid=p(valid, 4)),
           dict(new=p(new, 4)), dict(lpr=0), dict(n=0), dict(n=S + 1), dict(mask_stride=n - 1), dict(out=p(src, 4)),
           dict(mask=C.c_void_p(src.data_ptr())), dict(mask=C.c_void_p(out.data_ptr() + 16)), dict(new=p(src)), dict(new=p(out, 8)),
           dict(valid=p(new), new=p(new, 8)), dict(rows=1 << 31, S=1 << 20, n=300, mask_stride=300)]
    call = lambda a: pkg.lib().alacgpu_select_frames_device(ctx._ctx, a["src"], a["out"], a["rows"], a["lpr"], a["S"], a["n"], a["valid"],
                                                            a["mask"], a["mask_stride"], a["new"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    assert call({**good, "rows": 0}) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (new == 7).all() and (mask == 7).all()


def test_the_public_calls(gpu):
    import alac.net_amd as pkg

    torch, _ = gpu
    x = (8.0 + 6.0 * noise((3, 2, 30, 298), 4)).astype(np.float32)
    d = torch.from_numpy(x).cuda()
    lengths = [298, 123, -1]
    vad = pkg.EnergyVad.voxceleb()
    mask = pkg.vad_energy(d, vad, lengths)
    assert mask.dtype == torch.uint8 and mask.shape == (3, 298) and mask.is_contiguous()
    want = pkg.vad_host_f32(x, vad, lengths)
    assert np.array_equal(mask.cpu().numpy(), want) and 0 < want[0].sum() < 298
    assert torch.equal(pkg.vad_energy(d, vad, torch.tensor(lengths, device="cuda")), mask)
    assert np.array_equal(pkg.vad_energy(d[:, 0].contiguous(), pkg.EnergyVad(line=2)).cpu().numpy(), pkg.vad_host_f32(x[:, 0], pkg.EnergyVad(line=2)))
    assert np.array_equal(pkg.vad_energy(d[..., :-1], vad).cpu().numpy(), pkg.vad_host_f32(np.ascontiguousarray(x[..., :-1]), vad))
    y, new = pkg.select_host(x, want, lengths)
    got, glen = pkg.select_frames(d, mask, lengths)
    assert got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(x))
    assert same_bits(got.cpu().numpy(), y) and glen.dtype == torch.int64 and glen.tolist() == new.tolist() and new[2] == -1
    e = d.clone()
    res, glen = pkg.select_frames(e, mask.bool(), torch.tensor(lengths, device="cuda"), out=e)
    assert res is e and same_bits(e.cpu().numpy(), y) and glen.tolist() == new.tolist()
    got, glen = pkg.select_frames(d[:, 1].contiguous(), mask)                     # [B, lines, n], whole lines
    y2, new2 = pkg.select_host(x[:, 1], want)
    assert same_bits(got.cpu().numpy(), y2) and glen.tolist() == new2.tolist()
    assert pkg.vad_energy(d[:0], vad).shape == (0, 298) and pkg.select_frames(d[:0], mask[:0])[0].shape == (0, 2, 30, 298)
    for args in ((d.cpu(), vad), (d.double(), vad), (d, "vad"), (d, pkg.EnergyVad(line=30)), (d[..., ::2], vad), (d[0, 0], vad), (d, vad, [1, 2])):
        with pytest.raises(ValueError):
            pkg.vad_energy(*args)
    for args in ((d.cpu(), mask), (d, mask.cpu()), (d, mask[:, :-1]), (d, mask.float()), (d, mask, [1, 2]), (d, mask, None, d[..., :-1]),
                 (d, mask, None, d.double())):
        with pytest.raises(ValueError):
            pkg.select_frames(*args)
