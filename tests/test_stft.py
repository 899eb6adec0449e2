"""alacgpu_stft_device on the GPU against alac.net_amd/stft.py: bit for bit the float32 twin in front of the log and within the
derived bound of the float64 specification at every element; behind a log the device's logf (one unit in the last place) and
log10f (two) are not the twin's correctly rounded logarithm: there the kernel is within three units in the last place of the
twin and inside the bound.  A grid names the kernel's paths; then the properties that need no tolerance, and the C ABI's
refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 16000
CFG = [(512, 16, 40, 10, 14, 2)]


def signal(rows, L, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, L)).astype(np.float32)


def ulps(a, b):
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def rows_fb(K):
    """A band of one bin, a row of zeros, a dense row, a band ending at the Nyquist bin, zeros inside a band"""
    fb = np.zeros((5, K), dtype=np.float32)
    fb[0, 7] = 2.0
    fb[2] = np.linspace(0.1, 1.0, K)
    fb[3, K - 9:] = 1.0
    fb[4, [3, 9]] = -1.0, 1.0
    return fb


def grid():
    """name -> (Spectrogram arguments, L, rows); a tile is `stft.tile_frames`: 64 frames at 256 and 512 (32 for the complex
    kind at 512), 32 at 1024 (16 complex), 8 at 2048 (16 complex and with few lines)"""
    from alac.net_amd.features import mel_filterbank

    g = {}
    for N in (256, 512, 1024, 2048):
        g[f"{N}: the shortest row, one frame reflecting at both ends"] = (dict(n_fft=N, hop_length=N, power=2), N // 2 + 1, 2)
    # T' = tile - 1, tile, tile + 1 and 2 tile + 1: an odd last pair, a lone frame opening a tile
    for T in (31, 32, 33, 65):
        g[f"1024: {T} frames of a tile of 32"] = (dict(n_fft=1024, hop_length=20, power=1), 20 * (T - 1) + 3, 1)
    for T in (7, 8, 9, 17):
        g[f"2048 power: {T} frames of a tile of 8"] = (dict(n_fft=2048, hop_length=200, power=2), 200 * (T - 1) + 3, 1)
    for T in (15, 17, 33):
        g[f"2048 complex: {T} frames of a tile of 16"] = (dict(n_fft=2048, hop_length=80, power=None), 80 * (T - 1) + 1, 1)
    g["256: hop 1 at L = 300, five tiles of 64"] = (dict(n_fft=256, hop_length=1, power=2), 300, 1)
    g["512: hop = n_fft"] = (dict(n_fft=512, hop_length=512, power=1), 512 * 5 + 100, 2)
    g["512: a hop that does not divide the tile's span, complex, tile 32"] = (dict(n_fft=512, hop_length=37, power=None), 37 * 70, 1)
    g["256 complex, tile 64"] = (dict(n_fft=256, hop_length=20, power=None), 20 * 66, 1)
    g["1024 complex, tile 16"] = (dict(n_fft=1024, hop_length=100, power=None), 100 * 18, 2)
    g["256: win_length 1"] = (dict(n_fft=256, hop_length=50, win_length=1, power=1), 700, 1)
    g["512: win_length n_fft - 1"] = (dict(n_fft=512, hop_length=128, win_length=511, power=2), 1500, 1)
    g["512: win_length 400, a custom window"] = (dict(n_fft=512, hop_length=160, win_length=400,
                                                      window=np.hanning(400).astype(np.float32), power=2), 2000, 1)
    g["256: filterbank rows of every kind, on the power"] = (dict(n_fft=256, hop_length=64, filterbank=rows_fb(129)), 64 * 70, 2)
    g["1024: filterbank rows of every kind, on the magnitude"] = (dict(n_fft=1024, hop_length=256, power=1, filterbank=rows_fb(513)), 256 * 35, 1)
    g["2048: 256 mel lines, ln"] = (dict(n_fft=2048, hop_length=512, filterbank=mel_filterbank(22050, 2048, 256, norm=None), log="ln"), 512 * 18, 1)
    g["512: 80 mel lines, log10, the floor hit"] = (dict(n_fft=512, hop_length=160, filterbank=mel_filterbank(SR, 512, 80), log="log10",
                                                         floor=1.5), 3000, 2)
    g["256: ln of the magnitude, the floor hit"] = (dict(n_fft=256, hop_length=64, power=1, log="ln", floor=8.0), 1000, 2)
    return g


GRID = grid()


@pytest.mark.parametrize("name", list(GRID))
def test_the_kernel_is_the_twin_and_inside_the_bound(name):
    import torch

    import alac.net_amd as pkg

    kw, L, rows = GRID[name]
    spec = pkg.Spectrogram(SR, **kw)
    x = signal(rows, L, len(name))
    got = pkg.spectrogram(torch.from_numpy(x).cuda(), spec)
    torch.cuda.synchronize()
    T = int(spec.frames(L))
    assert got.shape == (rows, spec.n_mels, T) and got.dtype == torch.float32
    got = got.cpu().numpy()
    ref, bound = pkg.spectrogram_host(x, spec, bound=True)
    twin = pkg.spectrogram_host_f32(x, spec)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{name}: tile {spec.tile}, {T} frames, worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}, "
          f"differs from the twin in {int((got.view(np.int32) != twin.view(np.int32)).sum())} of {got.size}")
    assert np.isfinite(got).all()
    assert (err <= bound).all()
    if spec.log is None:
        assert np.array_equal(got.view(np.int32), twin.view(np.int32))
    else:
        floor = np.float32(spec.floor)
        at_floor = twin == (np.log(np.float64(floor)) if spec.log == "ln" else np.log10(np.float64(floor))).astype(np.float32)
        if "floor hit" in name:
            assert at_floor.any() and not at_floor.all()
        assert ulps(got, twin).max() <= 3


def test_the_grid_meets_the_tiles_it_names():
    from alac.net_amd.stft import tile_frames

    assert [tile_frames(256, 129, False), tile_frames(256, 258, False), tile_frames(512, 257, False), tile_frames(512, 514, False)] == [64, 64, 64, 32]
    assert [tile_frames(1024, 513, False), tile_frames(1024, 1026, False), tile_frames(2048, 1025, False), tile_frames(2048, 2050, False)] == [32, 16, 8, 16]
    assert tile_frames(2048, 256, True) == 16 and tile_frames(512, 80, True) == 64


def test_two_channels_a_stride_above_L_and_every_element_written():
    """The raw call on [2, 2, stride] with L < stride into an output poisoned beforehand: what lies behind L is not read"""
    import torch

    import alac.net_amd as pkg

    spec = pkg.Spectrogram(SR, 512, 100, power=None)
    L, S = 1234, 1500
    x = signal(4, S, 3).reshape(2, 2, S)
    other = x.copy()
    other[..., L:] = np.nan
    T = int(spec.frames(L))
    want = pkg.spectrogram_host_f32(np.ascontiguousarray(x[..., :L]), spec)
    window, table, _, _ = spec.device_tables(torch.device("cuda", 0))
    with pkg.AlacGpuContext(CFG) as ctx:
        for src in (x, other):
            out = torch.full((2, 2, spec.n_mels, T), float("nan"), device="cuda")
            out.view(torch.int32).fill_(0x5A5A5A5A)
            ctx.stft_device(torch.from_numpy(src).cuda(), 2, 2, S, L, 512, 100, window, table, 0, None, None, None, 0, 1e-10, out, T)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert not (got.view(np.int32) == 0x5A5A5A5A).any()
            assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_what_is_not_finite_stays_in_its_pair_and_is_never_hidden():
    import torch

    import alac.net_amd as pkg

    for kw in (dict(power=1), dict(power=None), dict(filterbank=rows_fb(129), log="ln")):
        spec = pkg.Spectrogram(SR, 256, 64, **kw)
        x = signal(2, 64 * 70, 9)                                          # 71 frames: two tiles
        clean = pkg.spectrogram(torch.from_numpy(x).cuda(), spec).cpu().numpy()
        y = x.copy()
        y[0, 64 * 6] = np.nan                                              # a tap of the frames 5 .. 8: the pairs (4, 5) .. (8, 9)
        y[0, 64 * 66 + 5] = np.inf                                         # of the frames 65 .. 68: the pairs (64, 65) .. (68, 69)
        got = pkg.spectrogram(torch.from_numpy(y).cuda(), spec).cpu().numpy()
        twin = pkg.spectrogram_host_f32(y, spec)
        touched = np.zeros(71, dtype=bool)
        touched[4:10] = touched[64:70] = True
        assert np.array_equal(got[1].view(np.int32), clean[1].view(np.int32))
        assert np.array_equal(got[0][:, ~touched].view(np.int32), clean[0][:, ~touched].view(np.int32))
        assert np.array_equal(np.isnan(got), np.isnan(twin)) and np.isnan(got[0][:, touched]).any(axis=0).all()
        finite = np.isfinite(twin)
        assert np.array_equal(got[~finite & ~np.isnan(twin)], twin[~finite & ~np.isnan(twin)])      # the infinities
        if spec.log is None:
            assert np.array_equal(got[finite].view(np.int32), twin[finite].view(np.int32))


def test_an_empty_batch_launches_nothing_and_the_refusals():
    import torch

    import alac.net_amd as pkg

    spec = pkg.Spectrogram(SR, 256, 64)
    out = pkg.spectrogram(torch.empty((0, 2, 500), device="cuda"), spec)
    assert out.shape == (0, 2, 129, 8)
    out, lens = pkg.spectrogram(torch.empty((0, 500), device="cuda"), spec, lengths=[])
    assert out.shape == (0, 129, 8) and lens.shape == (0,)
    out, lens = pkg.spectrogram(torch.zeros((3, 500), device="cuda"), spec, lengths=[500, 5, -1])
    assert lens.tolist() == [8, 1, -1]
    for bad in (torch.zeros(500), torch.zeros(500, device="cuda", dtype=torch.float64), torch.zeros((2, 128), device="cuda")):
        with pytest.raises(ValueError):
            pkg.spectrogram(bad, spec)
    with pytest.raises(ValueError):
        pkg.spectrogram(torch.zeros(500, device="cuda"), pkg.LogMel(SR))
    # the C ABI: every refusal is -1 and leaves `out` as it was
    fbspec = pkg.Spectrogram(SR, 256, 64, filterbank=rows_fb(129))
    window, table, d_bands, d_weights = fbspec.device_tables(torch.device("cuda", 0))
    x = torch.zeros((1, 1, 500), device="cuda")
    o = torch.empty((1, 1, 129, 8), device="cuda")
    o.view(torch.int32).fill_(0x5A5A5A5A)
    L = pkg.lib()
    dp, VP = pkg._dp, pkg._VP
    bands = np.ascontiguousarray(fbspec.bands, dtype=np.uint32)

    def call(gpu, **kw):
        a = dict(ctx=gpu._ctx, src=dp(x), rows=1, channels=1, stride=500, frames=500, n_fft=256, hop=64, window=dp(window), table=dp(table),
                 power=2, fb_lines=0, bands=None, d_bands=None, d_weights=None, log_mode=0, floor=1e-10, out=dp(o), out_frames=8)
        a.update(kw)
        if a["bands"] is not None:
            a["bands"] = a["bands"].ctypes.data_as(VP)
        return L.alacgpu_stft_device(*a.values(), None)

    with pkg.AlacGpuContext(CFG) as ctx:
        withfb = dict(fb_lines=5, bands=bands, d_bands=dp(d_bands), d_weights=dp(d_weights))
        wide, far, gap = bands.copy(), bands.copy(), bands.copy()
        wide[3, 1] += 1                              # a band past the Nyquist bin
        far[0, 0] = 130
        gap[4, 2] += 1                               # an offset that is not the sum of the counts before it
        many = np.zeros((257, 3), dtype=np.uint32)
        refused = [dict(ctx=None), dict(src=None), dict(window=None), dict(table=None), dict(out=None), dict(src=VP(x.data_ptr() + 2)),
                   dict(out=VP(o.data_ptr() + 1)), dict(table=VP(table.data_ptr() + 4)), dict(channels=0),
                   dict(n_fft=400), dict(n_fft=128), dict(n_fft=4096), dict(hop=0), dict(hop=257), dict(frames=128, out_frames=3),
                   dict(frames=501), dict(out_frames=7), dict(out_frames=9), dict(power=3), dict(power=-1), dict(log_mode=3),
                   dict(floor=0.0), dict(floor=float("inf")), dict(floor=float("nan")), dict(power=0, log_mode=1), dict(power=0, **withfb),
                   dict(withfb, bands=None), dict(withfb, d_bands=None), dict(withfb, d_weights=None), dict(withfb, bands=wide),
                   dict(withfb, bands=far), dict(withfb, bands=gap), dict(withfb, fb_lines=257, bands=many)]
        for kw in refused:
            assert call(ctx, **kw) == -1, kw
        torch.cuda.synchronize()
        assert bool((o.view(torch.int32) == 0x5A5A5A5A).all())
        assert call(ctx, rows=0) == 0 and call(ctx, rows=0, **withfb) == 0
        torch.cuda.synchronize()
        assert bool((o.view(torch.int32) == 0x5A5A5A5A).all())
        assert call(ctx, frames=129, out_frames=3) == 0                              # the shortest row is taken: [129, 3] of o
        o5 = torch.empty((1, 1, 5, 8), device="cuda")
        assert call(ctx, out=dp(o5), **withfb) == 0
        torch.cuda.synchronize()
        flat = o.view(torch.int32).flatten()
        assert not bool((flat[:387] == 0x5A5A5A5A).any()) and bool((flat[387:] == 0x5A5A5A5A).all())
