"""alacgpu_rir_shoebox_device on the GPU against alac.net_amd/rir.py: the kernel equals the float32 twin bit for bit on a grid of
the paths it takes, refused rows stay between good ones, `out=` slices are respected, and equal calls give equal bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 8000
ROOM = [3.0, 2.5, 2.0, 1.1, 0.9, 1.2, 2.0, 1.7, 0.8]
# the rows of every call of the grid: six different beta, a beta of 0 and of 1, a source 5 cm from the microphone (taps below 0
# are dropped), a room so large that no image arrives below K (zeros of length K), a room with one dimension 100 times another
ROWS = [(ROOM, [0.9, 0.5, 0.7, 0.95, 0.3, 0.6]), (ROOM, [0.0] * 6), (ROOM, [1.0] * 6), ([5, 4, 3, 2.5, 2, 1.5, 2.55, 2, 1.5], [0.7] * 6),
        ([400, 400, 50, 10, 10, 10, 300, 300, 10], [0.8] * 6), ([0.4, 40, 3, 0.1, 7, 1.2, 0.3, 9, 1.5], [0.85] * 6)]
# (K, W, max_order): K one below, at and one above a tile of 64 taps, K = 1, several tiles; W of 3, 41 and 81; orders None, 0, 3
GRID = [(63, 81, None), (64, 41, None), (65, 81, 3), (1, 3, None), (1, 81, None), (600, 81, None), (700, 3, None), (300, 41, 0),
        (129, 81, 3)]


def inputs():
    g = np.array([r[0] for r in ROWS], dtype=np.float64)
    b = np.array([r[1] for r in ROWS], dtype=np.float32)
    return g, b


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("K,W,order", GRID)
def test_kernel_equals_the_twin_bit_for_bit(K, W, order):
    import torch

    import alac.net_amd as pkg

    assert pkg.rir.TILE == 64
    g, b = inputs()
    want, wlen = pkg.rir_host_f32(g, b, FS, K, taps=W, max_order=order)
    got, lengths = pkg.simulate_rir(torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda(), FS, K, taps=W, max_order=order)
    assert got.shape == (len(ROWS), 1, K) and lengths.dtype == torch.int32
    assert lengths.cpu().tolist() == wlen.tolist() == [K] * len(ROWS)          # the far room too: zeros of the full length
    got = got.cpu().numpy()
    assert not got[4].any()
    if K >= 63:
        assert all(got[r].any() for r in (0, 1, 2, 3, 5))
    diff = bits(got) != bits(want)
    assert not diff.any(), (np.argwhere(diff)[:5], np.abs(got - want).max())


def test_refused_rows_between_good_ones():
    import torch

    import alac.net_amd as pkg

    bad = [ROOM[:3] + [float("nan")] + ROOM[4:], [3.0, 0.0, 2.0] + ROOM[3:], ROOM[:3] + [3.1] + ROOM[4:],
           [1e-5, 2.5, 2.0, 5e-6, 0.9, 1.2, 5e-6, 1.7, 0.8], [float("inf")] + ROOM[1:]]
    g = np.array([ROOM, bad[0], bad[1], ROOM, bad[2], bad[3], bad[4], ROOM], dtype=np.float64)
    b = np.full((8, 6), 0.8, dtype=np.float32)
    want, wlen = pkg.rir_host_f32(g, b, FS, 200)
    assert wlen.tolist() == [200, 0, 0, 200, 0, 0, 0, 200]
    got, lengths = pkg.simulate_rir(torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda(), FS, 200)
    assert lengths.cpu().tolist() == wlen.tolist()
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and not got[[1, 2, 4, 5, 6]].any() and got[0].any()
    # ... and `reverb` leaves the crops of the refused rows alone, bit for bit
    x = torch.randn(8, 1, 500, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
    y = pkg.reverb(x, torch.from_numpy(got).cuda(), None, lengths)
    for r in range(8):
        assert torch.equal(y[r], x[r]) == (wlen[r] == 0)


def test_out_slice_rows_0_and_equal_calls():
    import torch

    import alac.net_amd as pkg

    g, b = (torch.from_numpy(a).cuda() for a in inputs())
    K = 150
    first, flen = pkg.simulate_rir(g, b, FS, K)
    wide = torch.full((len(ROWS), 1, K + 37), float("nan"), device="cuda")
    got, lengths = pkg.simulate_rir(g, b, FS, K, out=wide[..., :K])
    assert got.data_ptr() == wide.data_ptr() and torch.equal(lengths, flen)
    assert torch.equal(got.view(torch.int32), first.view(torch.int32)) and bool(torch.isnan(wide[..., K:]).all())
    again, _ = pkg.simulate_rir(g, b, FS, K)
    assert torch.equal(again.view(torch.int32), first.view(torch.int32))
    none, nlen = pkg.simulate_rir(g[:0], b[:0], FS, K)
    assert none.shape == (0, 1, K) and nlen.shape == (0,)


def test_arguments_are_refused_before_any_device_work():
    import torch

    import alac.net_amd as pkg

    g, b = (torch.from_numpy(a).cuda() for a in inputs())
    for bad in (dict(taps=80), dict(taps=129), dict(max_order=-1), dict(sound_speed=0.0), dict(out=torch.empty(6, 1, 99, device="cuda")),
                dict(out=torch.empty(6, 1, 100, device="cuda", dtype=torch.float64))):
        with pytest.raises(ValueError):
            pkg.simulate_rir(g, b, FS, 100, **bad)
    for args in ((g.float(), b), (g, b.double()), (g[:, :8], b), (g, b[:3]), (g.cpu(), b), (g, b.cpu())):
        with pytest.raises(ValueError):
            pkg.simulate_rir(*args, FS, 100)
    with pytest.raises(ValueError):
        pkg.simulate_rir(g, b, FS, 0)
