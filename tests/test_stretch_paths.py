"""The paths of csrc/alac_stretch.hip that tests/test_stretch.py's grid does not reach, against the float32 twin
(alac.net_amd/pitch.py), bit for bit: bins that are exactly zero (`phasor()`'s branch for |z| not above 0), squares that are
subnormal or flush to zero, NaN and Inf inside the valid frames, `out_frames` below a row's new length (the clamps on `last`,
`count` and `valid_out`), terms at and around ALAC_STRETCH_MAX_TERM and non-positive ones, `valid` NULL and above `frames`,
chains of 500 output frames and outputs of 125 tiles, and the copy of rows with more than one tile per plane.  The harness is
tests/test_stretch.py's: a source that is the slice [..., :T] of longer planes, at or one float off 16 bytes, NaN behind every
length; the direct calls write into an output prefilled with NaN between guards of 0x5A bytes, as tests/test_reverb.py does."""
from fractions import Fraction as F

import numpy as np
import pytest

from test_stretch import RATE, bits

pytestmark = pytest.mark.gpu

FACTORS = (F(1, 2), F(2), F(9, 10), F(11, 10), F(200, 189))
GUARD = 64
NAN_BITS = np.array([np.nan], dtype=np.float32).view(np.int32)[0]
TINY = np.float32(2.0 ** -126)          # the least normal float32


@pytest.fixture(scope="module")
def gpu():
    import torch

    from alac.net_amd.resample import _context

    return torch, _context(0)


def noise(seed, B, C, T):
    """tests/test_stretch.py's signal: noise plus a sine"""
    rng = np.random.default_rng(seed)
    x = (0.25 * rng.standard_normal((B, C, T))).astype(np.float32)
    return x + (0.5 * np.sin(2 * np.pi * 440.0 / RATE * np.arange(T))).astype(np.float32)


def on_device(torch, x, layout, slack=16):
    """x as a device tensor that is the slice [..., :T] of planes of T + slack frames, NaN behind them; "offset": one float off
    16-byte alignment"""
    B, C, T = x.shape
    S = T + slack
    flat = torch.full((B * C * S + 4,), float("nan"), dtype=torch.float32, device="cuda")
    d = flat[1 if layout == "offset" else 0:][:B * C * S].view(B, C, S)[..., :T]
    assert (d.data_ptr() % 16 == 4) == (layout == "offset")
    d.copy_(torch.from_numpy(x))
    return d


def guarded(torch, n):
    """(raw, out): n floats of NaN between two guards of 0x5A bytes"""
    raw = torch.full(((n + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device="cuda").view(torch.float32)
    out = raw[GUARD:GUARD + n]
    out.fill_(float("nan"))
    return raw, out


def guards_stand(torch, raw, n):
    return bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all())


def untouched(a):
    """Whether every element still has the prefill's bits"""
    return bool((bits(a) == NAN_BITS).all())


def stretch_direct(gpu, x, terms, n_fft, out_frames, valid="frames", layout="stride", slack=5):
    """One ctx.time_stretch_device call over x [B, C, T] (numpy) with the terms [(p, q)] into planes of out_frames + slack
    frames between guards.  valid: a list, None (NULL) or "frames".  Returns (out [B, C, out_frames + slack] numpy, the new
    lengths) after checking the guards."""
    torch, ctx = gpu
    B, C, T = x.shape
    d = on_device(torch, x, layout)
    So = out_frames + slack
    raw, out = guarded(torch, B * C * So)
    d_p = torch.tensor([p for p, _ in terms], dtype=torch.int32, device="cuda")
    d_q = torch.tensor([q for _, q in terms], dtype=torch.int32, device="cuda")
    d_valid = None if valid is None else torch.tensor([T] * B if valid == "frames" else valid, dtype=torch.int64, device="cuda")
    d_new = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    ctx.time_stretch_device(d, out, B, C, d.stride(1), So, T, out_frames, d_p, d_q, d_valid, d_new, n_fft,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guards_stand(torch, raw, B * C * So), "a guard was written"
    assert np.array_equal(bits(d), bits(x)), "the source was written"
    return out.cpu().numpy().reshape(B, C, So), d_new.cpu().tolist()


def same_as_twin(torch, pkg, x, factors, lengths, n_fft, layout="stride"):
    """pkg.time_stretch on the device against time_stretch_host_f32, bit for bit; returns (the twin's y, the new lengths)"""
    want, want_lengths = pkg.time_stretch_host_f32(x, factors, lengths, n_fft)
    y, new_lengths = pkg.time_stretch(on_device(torch, x, layout), factors, lengths, n_fft)
    assert new_lengths.cpu().tolist() == want_lengths.tolist()
    assert y.shape == want.shape and np.array_equal(bits(y), bits(want))
    return want, want_lengths.tolist()


# ---- bins that are exactly zero -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [512, 1024])
def test_zero_bins_take_the_phasor_of_zero(gpu, n_fft):
    import alac.net_amd as pkg
    from alac.net_amd import pitch

    torch, _ = gpu
    N, H = n_fft, n_fft // 4
    T = 7 * N
    factors = [F(2), F(1, 2), F(200, 189), F(11, 10), F(9, 10), F(1, 2), F(2), F(9, 10)]
    x = np.zeros((8, 1, T), dtype=np.float32)
    sig = noise(n_fft, 2, 1, T)
    for b in (2, 3):                                        # signal, 3 n_fft frames of zeros, signal
        x[b] = sig[b - 2]
        x[b, :, 2 * N:5 * N] = 0
    x[4, 0, 3 * N + 77] = x[5, 0, 2 * N] = 1.0                 # a single impulse
    x[6:] = 0.5                                             # a constant
    # the premises, from the twin's own X
    frame_is_zero = []
    for b in range(8):
        Xr, Xi = pitch.analyse_host_f32(x[b], N)
        assert not Xr[:, -2:].any() and not Xi[:, -2:].any()
        frame_is_zero.append(~(Xr[0] != 0).any(axis=1) & ~(Xi[0] != 0).any(axis=1))
    assert frame_is_zero[0].all() and frame_is_zero[1].all()
    for b in (2, 3):
        z = frame_is_zero[b]
        assert z[10:19].all() and not z[:9].any() and not z[20:-2].any()       # the frames wholly inside the zeros
        p, q = factors[b].numerator, factors[b].denominator
        i, _ = pitch.steps(len(z) - 2, p, q)
        pairs = set(zip(z[i].tolist(), z[i + 1].tolist()))
        assert {(True, False), (False, True), (True, True), (False, False)} <= pairs   # zero as b, as a, as both (a factor above 1 skips no frame)
    for b, at in ((4, 3 * N + 77), (5, 2 * N)):
        z = frame_is_zero[b][:-2]
        t = np.arange(len(z))
        covers = (t * H - N // 2 < at) & (at < t * H + N // 2)                   # (w[0] = 0: a frame that starts at it is zero too)
        assert np.array_equal(~z, covers)
    Xr, Xi = pitch.analyse_host_f32(x[6], N)
    small = np.hypot(Xr[0, 3:-3, 3:].astype(np.float64), Xi[0, 3:-3, 3:]) <= 1e-5 * np.abs(Xr[0, 3:-3, 0:1])
    assert small.all()                                      # a constant: only rounding is left above bin 2 inside the row
    want, lens = same_as_twin(torch, pkg, x, factors, None, N, "offset")
    for b in (0, 1):
        assert lens[b] == pitch.stretched_frames(T, factors[b].numerator, factors[b].denominator)
        assert not want[b].any()                            # (the device's bits are the twin's: all zeros over the new length)
    assert np.isfinite(want).all() and want[2:].any(axis=2).all()


# ---- squares that are subnormal or underflow ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [512, 2048])
@pytest.mark.parametrize("exponent", [-40, -70, -85])
def test_squares_that_are_subnormal_or_flush_to_zero(gpu, n_fft, exponent):
    import alac.net_amd as pkg
    from alac.net_amd import pitch

    torch, _ = gpu
    T = 1400
    x = noise(exponent + n_fft, 2, 2, T) * np.float32(2.0 ** exponent)
    assert (np.abs(x[x != 0]) >= TINY).all()                 # the samples themselves are normal numbers
    for b in range(2):
        Xr, Xi = pitch.analyse_host_f32(x[b], n_fft)
        Xr, Xi = Xr[:, :-2], Xi[:, :-2]
        s = Xr * Xr + Xi * Xi                               # the twin's own float32 sum of squares
        nonzero = (Xr != 0) | (Xi != 0)
        assert nonzero.mean() > 0.99
        if exponent == -40:
            assert (s[nonzero] >= TINY).all()               # nothing special
        elif exponent == -70:
            assert ((s > 0) & (s < TINY)).mean() > 0.5      # most squares are subnormal
        else:
            assert (s[nonzero] == 0).mean() > 0.5           # the squares are zero, the bins are not
    want, _ = same_as_twin(torch, pkg, x, [F(11, 10), F(1, 2)], None, n_fft)
    assert np.isfinite(want).all()


# ---- NaN and Inf inside the valid frames ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_sample_stays_in_the_frames_that_cover_it(gpu, bad):
    import alac.net_amd as pkg
    from alac.net_amd import pitch

    torch, _ = gpu
    N, H, T, at = 512, 128, 2000, 1000
    factors = [F(9, 10), F(11, 10), F(2)]
    x = noise(5, 3, 2, T)
    clean, _ = pkg.time_stretch(on_device(torch, x, "stride"), factors, None, N)
    hit = x.copy()
    hit[1, 1, at] = bad
    want, lens = pkg.time_stretch_host_f32(hit, factors, None, N)
    y, _ = pkg.time_stretch(on_device(torch, hit, "stride"), factors, None, N)
    clean, y = clean.cpu().numpy(), y.cpu().numpy()
    for b in range(3):
        for c in range(2):
            if (b, c) != (1, 1):
                assert np.array_equal(bits(y[b, c]), bits(clean[b, c])), (b, c)
    got, twin = y[1, 1, :lens[1]], want[1, 1, :lens[1]]
    nan = np.isnan(twin)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(twin[~nan]))
    assert np.isfinite(twin[~nan]).all()
    # the frames that cover the sample, the output frames that read one of them, the samples those cover
    p, q = factors[1].numerator, factors[1].denominator
    t = np.arange(pitch.stft_frames(T, N))
    covers = (t * H - N // 2 <= at) & (at < t * H + N // 2)
    i, _ = pitch.steps(len(t), p, q)
    reads = np.nonzero(np.isin(i, t[covers]) | np.isin(i + 1, t[covers]))[0]
    first, behind = reads[0] * H - N // 2, reads[-1] * H + N // 2
    assert nan[first + 1:behind].any() and not nan[:first].any() and not nan[behind:].any()
    assert behind < lens[1] - 4 * H                          # the chain starts again from (1, 0) and runs on for frames


# ---- out_frames below a row's new length -----------------------------------------------------------------------------------------
def test_a_truncated_output_is_the_head_of_the_whole_one(gpu):
    from alac.net_amd import pitch

    N, H, T = 512, 128, 1000
    x = noise(11, len(FACTORS), 2, T)
    terms = [(f.numerator, f.denominator) for f in FACTORS]
    whole = [pitch.vocoder_host_f32(x[b], p, q, N) for b, (p, q) in enumerate(terms)]
    Ls = [w.shape[1] for w in whole]
    assert Ls == [500, 2000, 900, 1100, 1058]
    sizes = sorted({1, H - 1, H, 4 * H, 4 * H + 1} | {n + k for n in Ls for k in (-1, 0, 8)})
    for out_frames in sizes:
        got, new = stretch_direct(gpu, x, terms, N, out_frames, layout="offset" if out_frames % 2 else "stride")
        for b in range(len(terms)):
            n = min(Ls[b], out_frames)
            assert new[b] == n, (out_frames, b)
            assert np.array_equal(bits(got[b, :, :n]), bits(whole[b][:, :n])), (out_frames, b)
            assert not bits(got[b, :, n:out_frames]).any(), (out_frames, b)     # +0 from Ls up to out_frames
        assert untouched(got[:, :, out_frames:]), out_frames


# ---- the terms ----------------------------------------------------------------------------------------------------------------
def test_terms_up_to_the_limit_are_live_and_the_others_left_alone(gpu):
    from alac.net_amd import pitch

    N, T, M = 512, 700, 1 << 20
    live = [(M - 1, M), (M, M // 2 + 1), (M // 2 + 1, M), (18, 20), (9, 10)]
    alone = [(M + 1, M), (0, 5), (-3, 2), (5, 0), (7, 7)]
    for p, q in live + alone[:1]:
        assert F(1, 2) <= F(p, q) <= 2
    x = noise(13, len(live) + len(alone), 1, T)
    x[4] = x[3]                                             # the unreduced pair beside the reduced one
    valid = [T] * 10
    valid[6], valid[8] = T + 3, T - 100                        # (a row that is left alone reports min(valid, frames))
    whole = [pitch.vocoder_host_f32(x[b], p, q, N) for b, (p, q) in enumerate(live)]
    Ls = [w.shape[1] for w in whole]
    assert Ls == [pitch.stretched_frames(T, p, q) for p, q in live] and Ls[3] == Ls[4] == 630
    out_frames = max(Ls)
    got, new = stretch_direct(gpu, x, live + alone, N, out_frames, valid=valid)
    for b in range(len(live)):
        assert new[b] == Ls[b]
        assert np.array_equal(bits(got[b, :, :Ls[b]]), bits(whole[b])), live[b]
        assert not bits(got[b, :, Ls[b]:out_frames]).any()
    assert np.array_equal(bits(got[3]), bits(got[4]))
    for b in range(len(live), 10):
        assert new[b] == min(valid[b], T), (live + alone)[b]
        assert untouched(got[b]), (live + alone)[b]
    assert untouched(got[:, :, out_frames:])


# ---- the lengths ----------------------------------------------------------------------------------------------------------------
def test_no_lengths_and_lengths_above_the_frames_are_the_frames(gpu):
    import alac.net_amd as pkg

    torch, _ = gpu
    N, T = 512, 900
    x = noise(17, 3, 2, T)
    factors = [F(9, 10), F(11, 10), F(200, 189)]
    terms = [(f.numerator, f.denominator) for f in factors]
    want, lens = pkg.time_stretch_host_f32(x, factors, [T] * 3, N)
    Lo = want.shape[2]
    for valid in (None, [T + 9, T, T + 9]):
        got, new = stretch_direct(gpu, x, terms, N, Lo, valid=valid)
        assert new == lens.tolist()
        assert np.array_equal(bits(got[:, :, :Lo]), bits(want)) and untouched(got[:, :, Lo:])
    d = on_device(torch, x, "offset")
    a, la = pkg.time_stretch(d, factors, None, N)
    b, lb = pkg.time_stretch(d, factors, [T] * 3, N)
    assert np.array_equal(bits(a), bits(want)) and np.array_equal(bits(b), bits(want))
    assert la.cpu().tolist() == lb.cpu().tolist() == lens.tolist()


# ---- long rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, T, factor, n_fft", [(1, 32000, F(2), 512), (2, 9000, F(200, 189), 2048)])
def test_long_chains_and_many_tiles(gpu, C, T, factor, n_fft):
    import alac.net_amd as pkg
    from alac.net_amd import pitch

    torch, _ = gpu
    x = noise(T, 1, C, T)
    want, lens = same_as_twin(torch, pkg, x, [factor], None, n_fft, "offset")
    frames = pitch.vocoder_frames(pitch.stft_frames(T, n_fft), factor.numerator, factor.denominator)
    if n_fft == 512:
        assert frames == 502 and lens == [64000] and -(-lens[0] // (4 * 128)) == 125
    assert np.isfinite(want).all()


# ---- the copy of rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("frames", [4095, 4096, 4097, 8200])
def test_copy_rows_copies_the_valid_frames_and_nothing_else(gpu, frames, C):
    torch, ctx = gpu
    valid = [-1, 0, 1, 4096, 4097, frames, frames + 5]
    B, S, So = len(valid), frames + 3, frames + 6
    rng = np.random.default_rng(frames + C)
    x = rng.integers(-2 ** 31, 2 ** 31, size=(B, C, frames), dtype=np.int64).astype(np.int32).view(np.float32)    # any bits at all
    flat = torch.full((B * C * S + 4,), float("nan"), dtype=torch.float32, device="cuda")
    d = flat[1:][:B * C * S].view(B, C, S)
    assert d.data_ptr() % 16 == 4
    d[..., :frames].view(torch.int32).copy_(torch.from_numpy(x.view(np.int32)))
    raw, out = guarded(torch, B * C * So)
    ctx.copy_rows_device(d, out, B, C, S, So, frames, torch.tensor(valid, dtype=torch.int64, device="cuda"),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guards_stand(torch, raw, B * C * So), "a guard was written"
    got = out.cpu().numpy().reshape(B, C, So)
    for b, v in enumerate(valid):
        n = min(max(v, 0), frames)
        assert np.array_equal(bits(got[b, :, :n]), x[b, :, :n].view(np.int32)), (b, v)
        assert untouched(got[b, :, n:]), (b, v)
    assert np.array_equal(bits(d[..., :frames]), x.view(np.int32))


def test_copy_rows_refuses_bad_arguments_and_enqueues_nothing(gpu):
    import alac.net_amd as pkg

    torch, ctx = gpu
    rows, C, S, T = 3, 2, 16, 10
    src = torch.zeros(rows * C * S + 8, device="cuda")
    out = torch.full((rows * C * S + 8,), 7.0, device="cuda")
    valid = torch.full((rows,), T, dtype=torch.int64, device="cuda")
    base = dict(d_src=src.data_ptr(), d_out=out.data_ptr(), rows=rows, channels=C, src_stride=S, out_stride=S, frames=T,
                d_valid=valid.data_ptr(), stream=None)
    extent = 4 * ((rows * C - 1) * S + T)
    cases = [dict(frames=0), dict(frames=S + 1), dict(src_stride=T - 1), dict(out_stride=T - 1), dict(d_valid=None),
             dict(d_out=base["d_src"]), dict(d_out=base["d_src"] + 4), dict(d_out=base["d_src"] + extent - 4),
             dict(d_src=None), dict(d_out=None), dict(channels=0), dict(d_src=base["d_src"] + 2), dict(d_valid=base["d_valid"] + 4)]
    fn = pkg.lib().alacgpu_copy_rows_device
    for change in cases:
        assert fn(ctx._ctx, *dict(base, **change).values()) == -1, change
    assert fn(None, *base.values()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((src == 0).all())
    # ... and the same arguments unchanged are a call, as is one of no rows
    assert fn(ctx._ctx, *dict(base, rows=0).values()) == 0
    assert fn(ctx._ctx, *base.values()) == 0
    torch.cuda.synchronize()
    got = out[:rows * C * S].view(rows, C, S).cpu()
    assert bool((got[..., :T] == 0).all()) and bool((got[..., T:] == 7.0).all()) and bool((out[rows * C * S:] == 7.0).all())


# ---- the pitch shift across a tile of the copy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("turn", [0, 1])
def test_pitch_shift_across_a_copy_tile(gpu, turn):
    import alac.net_amd as pkg

    torch, _ = gpu
    T, lengths = 5000, [5000, 4097, 300]
    ratios = [(F(55, 49), F(49, 55))[(b + turn) % 2] for b in range(3)]
    x = noise(19 + turn, 3, 2, T)
    for b, v in enumerate(lengths):
        x[b, :, v:] = np.nan
    want = pkg.pitch_shift_host_f32(x, ratios, RATE, lengths, 512)
    d = on_device(torch, x, "offset" if turn else "stride")
    y = pkg.pitch_shift(d, ratios, RATE, lengths, 512)
    assert y is not d and np.array_equal(bits(d), bits(x))
    assert np.array_equal(bits(y), bits(want))
    for b, v in enumerate(lengths):
        assert np.isfinite(want[b, :, :v]).all() and untouched(want[b, :, v:])
    same = pkg.pitch_shift(d, ratios, RATE, torch.tensor(lengths, device="cuda"), 512, out=d)
    assert same is d and np.array_equal(bits(d), bits(want))
