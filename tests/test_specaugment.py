"""alacgpu_specaugment_device on the GPU against the float32 twin of alac.net_amd/augment.py, bit for bit: every frame count at
which the kernel takes another path (fewer frames than a 128-bit access, a wave's 64 lanes, the threshold between the two
mappings, the staging limit), 1, 5 and 80 bins, one and two channels, contiguous lines and the slice [..., :N] of N + 1 (an
odd stride: unaligned lines), out of place and in place, with draws built by hand.  The data of warped rows is finite below
tau; everywhere else it carries NaNs with payloads, which have to come back as the bits they were."""
import numpy as np
import pytest

from test_features import header_constant

pytestmark = pytest.mark.gpu

WAVE_MAX = header_constant("ALAC_AUG_WAVE_MAX", "alac_augment.h")
LDS_MAX = header_constant("ALAC_AUG_LDS_MAX", "alac_augment.h")
W = 2
FILL = -1.25
SENTINEL = 777.0
# (N, M, C): every N with 5 bins and two channels; 1 and 80 bins and one channel at the sizes of each mapping
SHAPES = [(n, 5, 2) for n in (1, 2, 3, 4, 5, 63, 64, 65, 201, WAVE_MAX, WAVE_MAX + 1, LDS_MAX)] + \
         [(201, 80, 1), (64, 1, 1), (WAVE_MAX + 1, 1, 2), (3000, 80, 1)]


def lengths_for(N):
    """-1, 0, 1, 2, 3, 2 W + 2, 2 W + 3, N and N + 7 in batches of at most 4 rows (of the longest lines: one batch)"""
    if N == LDS_MAX:
        return [[N, N + 7, 2 * W + 3, -1]]
    return [[-1, N, 0, 1], [2, 3, N + 7, 2 * W + 2], [2 * W + 3, N, max(N - 1, 0), N // 2]]


def draws_for(taus, M, shift):
    """Draws by hand for rows of `taus` valid frames, row b taking kind (b + shift) % 6:
      0  nothing at all -- next to 1, a row with everything
      1  c = tau - 2 -> c' = 1; a mask of width 0, the last bin; the last frame, a mask of width 0
      2  c = 1 -> c' = tau - 2; no frequency mask; two time masks that overlap
      3  c = tau // 2 -> c' = c + W (or c - W at the end); the first bin, the last two; the first quarter, a span over tau
      4  no warp; a middle bin and a mask that runs past the last bin; a mask from in front of frame 0, one past tau
      5  no warp; every bin masked; every frame masked"""
    B = len(taus)
    warp, freq, time = np.zeros((B, 2), np.int32), np.zeros((B, 2, 2), np.int32), np.zeros((B, 2, 2), np.int32)
    for b, tau in enumerate(taus):
        kind = (b + shift) % 6
        if kind == 1:
            warp[b], freq[b], time[b] = (tau - 2, 1), [(0, 0), (M - 1, 1)], [(tau - 1, 1), (3, 0)]
        elif kind == 2:
            warp[b], time[b] = (1, tau - 2), [(tau // 4, tau // 2), (tau // 3, tau // 2)]
        elif kind == 3:
            c = tau // 2
            warp[b] = (c, c + W if c + W <= tau - 2 else c - W)
            freq[b], time[b] = [(0, 1), (M - 2, 2)], [(0, tau // 4), (tau - 3, 9)]
        elif kind == 4:
            freq[b], time[b] = [(M // 2, 1), (M - 1, 5)], [(-2, 4), (tau - 1, 9)]
        elif kind == 5:
            freq[b], time[b] = [(0, M), (0, 0)], [(0, tau), (0, 0)]
    return warp, freq, time


def warped_rows(warp, taus):
    return np.array([c != c1 and 1 <= c <= t - 2 and 1 <= c1 <= t - 2 for (c, c1), t in zip(warp.tolist(), taus)])


def payloads(shape, seed):
    """NaNs whose payloads differ"""
    bits = np.random.default_rng(seed).integers(1, 1 << 22, shape, dtype=np.int64) | 0x7FC00000
    return bits.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("N,M,C", SHAPES)
def test_the_kernel_is_the_twin_bit_for_bit(N, M, C):
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(N * 7 + M + C)
    saw_warp = saw_plain = False
    for shift, lens in enumerate(lengths_for(N)):
        B = len(lens)
        taus = [min(max(v, 0), N) for v in lens]
        warp, freq, time = draws_for(taus, M, shift)
        on = warped_rows(warp, taus)
        saw_warp |= bool(on.any())
        saw_plain |= bool((~on).any())
        x = rng.standard_normal((B, C, M, N)).astype(np.float32)
        nan = payloads(x.shape, N + shift)
        for b in range(B):
            if on[b]:
                x[b, ..., taus[b]:] = nan[b, ..., taus[b]:]            # behind tau: never read
            else:
                x[b].reshape(-1)[::3] = nan[b].reshape(-1)[::3]        # a row without a warp is never computed with
        want = pkg.specaugment_host_f32(x, warp, freq, time, lens, fill=FILL)
        wbits = torch.from_numpy(want.view(np.int32))
        xbits = torch.from_numpy(x.view(np.int32))
        draws = tuple(torch.from_numpy(t).cuda() for t in (warp, freq, time))
        how = (pkg.SpecAugment(time_warp=W, fill=FILL), draws)
        d_lens = torch.tensor(lens, device="cuda")
        for sliced in (False, True):
            def tensor(fill_with):
                base = torch.full((B, C, M, N + 1 if sliced else N), SENTINEL, device="cuda")
                view = base[..., :N]
                if fill_with is not None:
                    view.view(torch.int32).copy_(torch.from_numpy(fill_with.view(np.int32)).cuda())     # (as integers: the bits)
                return base, view
            # out of place: the twin, the source unchanged, nothing behind a line written
            xb, xv = tensor(x)
            ob, ov = tensor(None)
            assert pkg.spec_augment(xv, how, d_lens, out=ov) is ov
            assert torch.equal(ov.contiguous().view(torch.int32).cpu(), wbits), (N, M, C, lens, sliced, "out of place")
            assert torch.equal(xv.contiguous().view(torch.int32).cpu(), xbits)
            if sliced:
                assert bool((ob[..., N] == SENTINEL).all()) and bool((xb[..., N] == SENTINEL).all())
            got = pkg.spec_augment(xv, how, lens)                       # a new tensor of x's layout, lengths as a list
            assert got.stride() == xv.stride() and torch.equal(got.contiguous().view(torch.int32).cpu(), wbits)
            # in place
            assert pkg.spec_augment(xv, how, d_lens, out=xv) is xv
            inplace = xv.contiguous().view(torch.int32).cpu()
            assert torch.equal(inplace, wbits), (N, M, C, lens, sliced, "in place")
            if sliced:
                assert bool((xb[..., N] == SENTINEL).all())
            for b in np.nonzero(~on)[0]:                               # what is not masked in a row without a warp: the same bits
                same = want[b] != np.float32(FILL)
                assert torch.equal(inplace[b][torch.from_numpy(same)], xbits[b][torch.from_numpy(same)])
    assert saw_plain and (saw_warp or N < 4)


def test_masks_alone_have_no_staging_limit_and_a_triple_fills_with_zero():
    import torch

    import alac.net_amd as pkg

    N, M = LDS_MAX + 5, 3
    x = np.random.default_rng(1).standard_normal((2, 1, M, N)).astype(np.float32)
    freq = np.array([[(1, 1)], [(0, 0)]], np.int32)
    time = np.array([[(N - 10, 10), (5, 0)], [(100, LDS_MAX), (0, 1)]], np.int32)
    lens = [N, N - 3]
    d = tuple(torch.from_numpy(t).cuda() for t in (freq, time))
    want = torch.from_numpy(pkg.specaugment_host_f32(x, None, freq, time, lens))
    d_x = torch.from_numpy(x).cuda()
    assert torch.equal(pkg.spec_augment(d_x, (None, *d), lens).cpu(), want)
    assert torch.equal(pkg.spec_augment(d_x, (pkg.SpecAugment(time_warp=0), (torch.zeros(2, 2, dtype=torch.int32, device="cuda"), *d)), lens).cpu(), want)
    assert torch.equal(pkg.spec_augment(d_x, (None, *d), lens, out=d_x).cpu(), want)
    # a SpecAugment alone draws from the device's default generator
    spec = pkg.SpecAugment(time_warp=W, time_ratio=0.2, fill=FILL)
    y = torch.from_numpy(x[..., :300].copy()).cuda()
    d_lens = torch.tensor([300, 120], device="cuda")
    torch.cuda.manual_seed(3)
    a = pkg.spec_augment(y, spec, d_lens)
    torch.cuda.manual_seed(3)
    draws = spec.draw(M, d_lens)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in draws)
    want = pkg.specaugment_host_f32(x[..., :300], *(t.cpu().numpy() for t in draws), [300, 120], fill=FILL)
    assert torch.equal(a.cpu(), torch.from_numpy(want)) and not torch.equal(a, y)


def test_what_cannot_be_augmented_is_refused_before_any_device_work():
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import _context

    x = torch.zeros(2, 1, 4, LDS_MAX + 1, device="cuda")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    ok = (z(2, 2), z(2, 1, 2), z(2, 1, 2))
    small = torch.zeros(2, 1, 4, 50, device="cuda")
    assert pkg.spec_augment(small, ok).shape == small.shape
    bad = [
        (x, pkg.SpecAugment(time_warp=1)), (x, ok), (x, (pkg.SpecAugment(time_warp=1), ok)),          # a warp above the staging limit
        (small.transpose(2, 3), ok), (small[..., ::2], ok), (small.expand(2, 3, 4, 50), ok),          # layouts _lines rejects
        (small, tuple(t.cpu() for t in ok)), (small.cpu(), ok),                                        # another device
        (small, (z(3, 2), ok[1], ok[2])), (small, (z(2, 3), ok[1], ok[2])), (small, (ok[0], z(2, 2), ok[2])),
        (small, (ok[0], ok[1], z(2, 1, 3))), (small, (ok[0].long(), ok[1], ok[2])), (small, (ok[0], ok[1].float(), ok[2])),
        (small, (ok[0], ok[1])), (small, (ok[0], None, ok[2])), (small, "spec"), (small, None), (small[0], ok), (small.double(), ok),
        (small, (ok[0], ok[1], z(2, 1025, 2))),
    ]
    for t, how in bad:
        with pytest.raises(ValueError):
            pkg.spec_augment(t, how)
    for kw in (dict(lengths=[1]), dict(lengths=torch.zeros(2)), dict(out=torch.zeros(2, 1, 4, 51, device="cuda")),
               dict(out=torch.zeros(2, 1, 4, 51, device="cuda")[..., :50]), dict(out=small.double())):
        with pytest.raises(ValueError):
            pkg.spec_augment(small, ok, **kw)
    assert not bool(small.any())
    # the library itself refuses the same
    ctx = _context(0)
    with pytest.raises(pkg.AlacGpuError):
        ctx.specaugment_device(x, x, 2, 1, 4, LDS_MAX + 1, LDS_MAX + 1, None, ok[0], None, None, 0.0)
    with pytest.raises(pkg.AlacGpuError):
        ctx.specaugment_device(small, small, 2, 1, 4, 50, 50, None, None, None, None, float("nan"))
    ctx.specaugment_device(x, x, 2, 1, 4, LDS_MAX + 1, LDS_MAX + 1, None, None, ok[1], ok[2], 0.0)     # masks alone: taken
    torch.cuda.synchronize()
