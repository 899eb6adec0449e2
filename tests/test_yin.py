"""alacgpu_yin_device on the GPU, bit for bit its float32 twin in numpy (yin.yin_host_f32) on every output element, on the
smallest shapes that reach each path of csrc/alac_yin.hip, then `alac.yin`.

Every call goes through `run`: the input is the slice [..., :T] of a tensor whose slack behind every plane is NaN, the output
lies between guards; the guards, the input's bytes and the absence of a NaN in the output -- a read past a row would bring one
-- are checked after every call."""
import numpy as np
import pytest

from test_yin_spec import mixed_signal, same_bits, voiced_noise

pytestmark = pytest.mark.gpu

SLACK = 7          # (odd: the planes then start off 16-byte boundaries)
GUARD = 64


def run(torch, pkg, x, spec, lengths=None, slack=SLACK, give_out=False):
    """alac.yin over x [B, C, T] (numpy) as the slice of a tensor with `slack` NaNs behind every plane; returns the track as
    numpy"""
    B, C, T = x.shape
    src = np.full((B, C, T + slack), np.nan, dtype=np.float32)
    src[..., :T] = x
    d_src = torch.from_numpy(src).cuda()
    view = d_src[..., :T] if slack else d_src
    n = int(spec.frames(T))
    out = None
    if give_out:
        raw = torch.full((B * C * 2 * n + 2 * GUARD,), 12345.0, dtype=torch.float32, device="cuda")
        out = raw[GUARD:GUARD + B * C * 2 * n].view(B, C, 2, n)
    got = pkg.yin(view, spec, lengths, out=out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, C, 2, n) and got.dtype == torch.float32
    if give_out:
        assert got.data_ptr() == out.data_ptr()
        assert bool((torch.cat([raw[:GUARD], raw[GUARD + B * C * 2 * n:]]) == 12345.0).all()), "a guard was written"
    assert np.array_equal(d_src.cpu().numpy(), src, equal_nan=True), "the samples were written"
    got = got.cpu().numpy()
    assert not np.isnan(got).any(), "a NaN: something behind a row was read"
    return got


def check(torch, pkg, x, spec, lengths=None, **kw):
    from alac.net_amd.yin import yin_host_f32

    got = run(torch, pkg, x, spec, lengths, **kw)
    want = yin_host_f32(x, spec, lengths)
    assert same_bits(got, want), (spec, np.argwhere(got.view(np.int32) != want.view(np.int32))[:5])
    if lengths is not None:                 # zeros at and behind every row's frame count
        counts = spec.lengths(np.clip(np.asarray(lengths), 0, x.shape[-1]))
        for b, n in enumerate(counts):
            assert not got[b, :, :, n:].any()
    return got


# (rate, win_length, hop, fmin, fmax): tau_max 128 (a multiple of 64), 267 and 160; a hop that is no multiple of 4 takes the
# kernel without 16-byte LDS reads
GRID = [(16000, 64, 40, 125.0, 400.0), (16000, 512, 160, 60.0, 400.0), (8000, 64, 50, 50.0, 400.0), (8000, 512, 81, 50.0, 380.0)]


@pytest.mark.parametrize("rate, win, hop, fmin, fmax", GRID)
@pytest.mark.parametrize("center", [True, False])
def test_the_kernel_is_the_twin_bit_for_bit(rate, win, hop, fmin, fmax, center):
    """B = 3, C = 2 with lengths [0, 37, T]; T such that T' is one more than a multiple of the tile (centred) or one less
    (not centred, whatever align_length gives is checked below)"""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.yin import tile_frames

    spec = pkg.Yin(rate, win, hop, fmin, fmax, 0.15, center=center, align_length=None if center else 100)
    tile = tile_frames(spec)
    T = 2 * tile * hop + (3 if center else 100 - 2 * hop + 3)
    assert spec.frames(T) == (2 * tile + 1 if center else 2 * tile - 1)
    x = voiced_noise(3, 2, T, rate, seed=win + hop)
    check(torch, pkg, x, spec, [0, 37, T])
    check(torch, pkg, x, spec, None, give_out=True)


def test_lengths_at_the_edges_of_the_frame_counts():
    """A length that is a multiple of hop, one below it, align_length itself and one below align_length (no frame), -1 and
    more than T"""
    import torch

    import alac.net_amd as pkg

    T = 1000
    x = voiced_noise(6, 1, T, 16000, seed=5)
    for spec in (pkg.Yin(16000, 64, 40, 125.0, 400.0), pkg.Yin(16000, 64, 40, 125.0, 400.0, center=False, align_length=400)):
        got = check(torch, pkg, x, spec, [400, 399, 440, 439, -1, T + 5])
        assert got.shape[-1] == spec.frames(T)
    assert pkg.Yin(16000, 64, 40, 125.0, 400.0, center=False, align_length=400).lengths(np.array([400, 399])).tolist() == [1, 0]


def test_contiguous_input_two_dimensions_and_device_lengths():
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.yin import yin_host_f32

    spec = pkg.Yin(16000, 64, 40, 125.0, 400.0)
    x = voiced_noise(2, 1, 777, 16000, seed=9)
    check(torch, pkg, x, spec, None, slack=0)
    got = pkg.yin(torch.from_numpy(x[:, 0]).cuda(), spec, torch.tensor([500, 777], device="cuda"))
    assert tuple(got.shape) == (2, 2, spec.frames(777))
    assert same_bits(got.cpu().numpy(), yin_host_f32(x[:, 0], spec, [500, 777]))


def test_silence_constants_and_a_nan_sample():
    """Silent and constant rows are (0, 1) in every frame of theirs; a NaN sample reaches the frames whose span holds it, as
    the twin says, and no other"""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.yin import yin_host_f32

    spec = pkg.Yin(16000, 64, 40, 125.0, 400.0)
    T = 1200
    x = voiced_noise(3, 1, T, 16000, seed=3)
    x[0] = 0.0
    x[1] = 0.25
    x[1, 0, T - 300:] = 0.0                 # (a constant whose end is a step: those frames are not silent)
    got = check(torch, pkg, x, spec)
    assert (got[0, 0, 0] == 0).all() and (got[0, 0, 1] == 1).all()
    inner = slice(3, 15)
    assert (got[1, 0, 0, inner] == 0).all() and (got[1, 0, 1, inner] == 1).all()
    # the NaN: the harness's own check of the output does not apply, so the call is made by hand
    x[2, 0, 600] = np.nan
    d = torch.from_numpy(x).cuda()
    y = pkg.yin(d, spec).cpu().numpy()
    want = yin_host_f32(x, spec)
    # (a NaN is a NaN: its sign and payload are no part of the specification)
    assert np.array_equal(np.isnan(y), np.isnan(want)), np.argwhere(np.isnan(y) != np.isnan(want))[:5]
    assert same_bits(np.nan_to_num(y, nan=-1.0), np.nan_to_num(want, nan=-1.0)), np.argwhere(np.nan_to_num(y, nan=-1.0) != np.nan_to_num(want, nan=-1.0))[:5]
    hit = np.isnan(y[2, 0, 1])
    t = np.arange(y.shape[-1])
    s = spec.first + t * spec.hop_length
    holds = (s <= 600) & (600 < s + spec.span)
    assert hit.any() and not (hit & ~holds).any() and not np.isnan(y[:2]).any()
    assert same_bits(y[2, 0][:, ~holds], got[2, 0][:, ~holds])


def test_empty_batches_and_rows_without_samples():
    import torch

    import alac.net_amd as pkg

    spec = pkg.Yin(16000, 64, 40, 125.0, 400.0)
    assert tuple(pkg.yin(torch.empty((0, 2, 500), device="cuda"), spec).shape) == (0, 2, 2, 13)
    got = pkg.yin(torch.empty((2, 1, 0), device="cuda"), spec)                     # T = 0, centred: one frame of silence
    assert tuple(got.shape) == (2, 1, 2, 1) and got[:, :, 0].tolist() == [[[0.0]], [[0.0]]] and got[:, :, 1].tolist() == [[[1.0]], [[1.0]]]
    snip = pkg.Yin(16000, 64, 40, 125.0, 400.0, center=False, align_length=400)
    assert tuple(pkg.yin(torch.zeros((2, 1, 399), device="cuda"), snip).shape) == (2, 1, 2, 0)
    with pytest.raises(ValueError):
        pkg.yin(torch.zeros((2, 1, 399), device="cuda", dtype=torch.float64), spec)
    with pytest.raises(ValueError):
        pkg.yin(torch.zeros((2, 1, 800), device="cuda")[..., ::2], spec)
    with pytest.raises(ValueError):
        pkg.yin(torch.zeros((2, 1, 400), device="cuda"), spec, out=torch.zeros((2, 1, 2, 3), device="cuda"))


def test_the_mixed_signal_through_the_kernel():
    """The issue's signal: 51 frames, 35 voiced, and the kernel's bits are the twin's"""
    import torch

    import alac.net_amd as pkg

    spec = pkg.Yin(16000, 512, 160, 60, 400, 0.1)
    got = check(torch, pkg, mixed_signal()[None, None, :], spec)
    assert got.shape == (1, 1, 2, 51) and int(spec.voiced(got).sum()) == 35
