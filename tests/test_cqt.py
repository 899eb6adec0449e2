"""alacgpu_cqt_device on the GPU against alac.net_amd/cqt.py: within the derived bound of the float64 specification at every
element, and bit for bit the float32 twin -- but behind a log, where the device's logf (one unit in the last place) and log10f
(two) are not the twin's correctly rounded logarithm: there the kernel is within three units in the last place of the twin, and
everything else holds.  A grid names the kernel's paths; then the properties that need no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR, FMIN = 2000, 50.0          # N_0 = 673 at 12 bins an octave, 2058 at 36

# name -> (ConstantQ arguments behind the rate, L, rows)
GRID = {
    "two blocks, the second partial; odd and even N_k in a block": (dict(hop_length=64, n_bins=30), 1500, 2),
    "fewer bins than a block, an odd hop": (dict(hop_length=63, n_bins=7), 1000, 2),
    "whole blocks, 24 an octave, filter_scale 0.5": (dict(hop_length=64, n_bins=32, bins_per_octave=24, filter_scale=0.5), 1200, 1),
    "24 an octave, filter_scale 1": (dict(hop_length=96, n_bins=20, bins_per_octave=24), 2000, 1),
    "36 an octave, filter_scale 1": (dict(hop_length=128, n_bins=40, bins_per_octave=36), 3000, 1),
    "36 an octave, filter_scale 0.5": (dict(hop_length=128, n_bins=40, bins_per_octave=36, filter_scale=0.5), 2000, 1),
    "12 an octave, filter_scale 0.5, unscaled": (dict(hop_length=50, n_bins=17, filter_scale=0.5, scale=False), 900, 2),
    "hop 1: seven tiles": (dict(hop_length=1, n_bins=20), 200, 1),
    "a hop above N_0": (dict(hop_length=700, n_bins=18), 3000, 2),
    "L below N_0: mostly padding": (dict(hop_length=16, n_bins=30), 100, 2),
    "L = 1": (dict(hop_length=64, n_bins=30), 1, 2),
    "three tiles of 32 frames": (dict(hop_length=64, n_bins=18), 64 * 70, 1),
    "tiles of 21 frames: the span of 32 does not fit": (dict(hop_length=2000, n_bins=16), 2000 * 45, 1),
    "power 2": (dict(hop_length=64, n_bins=30, power=2), 1000, 2),
    "ln, the floor hit": (dict(hop_length=64, n_bins=30, log="ln", floor=0.3), 1000, 2),
    "log10 of the power, the floor hit": (dict(hop_length=64, n_bins=30, log="log10", power=2, floor=0.05), 1000, 2),
}


def signal(rows, L, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, L)).astype(np.float32)
    if rows > 1 and L > 8:
        x[1, L // 2:] = 0            # a row that ends in silence, as a crop's padding
    return x


def ulps(a, b):
    """How many float32 values apart a and b are, elementwise (finite values)"""
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("name", list(GRID))
def test_the_kernel_is_the_twin_and_inside_the_bound(name):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.cqt import tile_frames

    kw, L, rows = GRID[name]
    spec = pkg.ConstantQ(SR, f_min=FMIN, **kw)
    x = signal(rows, L, len(name))
    got = pkg.cqt(torch.from_numpy(x).cuda(), spec)
    torch.cuda.synchronize()
    T = int(spec.frames(L))
    assert got.shape == (rows, spec.n_bins, T) and got.dtype == torch.float32
    got = got.cpu().numpy()
    ref, bound = pkg.cqt_host(x, spec, bound=True)
    twin = pkg.cqt_host_f32(x, spec)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{name}: N_0 {int(spec.lens[0])}, tile {tile_frames(int(spec.lens[0]), spec.hop_length)}, {T} frames, "
          f"worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}, "
          f"differs from the twin in {int((got.view(np.int32) != twin.view(np.int32)).sum())} of {got.size}")
    assert np.isfinite(got).all()
    assert (err <= bound).all()
    if spec.log is None:
        assert np.array_equal(got.view(np.int32), twin.view(np.int32))
    else:
        floor = np.float32(spec.floor)
        at_floor = twin == (np.log(np.float64(floor)) if spec.log == "ln" else np.log10(np.float64(floor))).astype(np.float32)
        assert at_floor.any() and not at_floor.all()                   # the floor is hit, and not everywhere
        assert ulps(got, twin).max() <= 3


def test_a_frame_does_not_depend_on_where_it_sits():
    import torch

    import alac.net_amd as pkg

    spec = pkg.ConstantQ(SR, hop_length=64, f_min=FMIN, n_bins=30)
    x = signal(1, 64 * 40, 5)
    a = pkg.cqt(torch.from_numpy(x).cuda(), spec)
    for shift in (1, 17, 33):                                           # frames: across tiles and lanes
        y = np.concatenate([np.zeros((1, 64 * shift), np.float32), x], axis=1)
        b = pkg.cqt(torch.from_numpy(y).cuda(), spec)
        # frame t of x reads the samples frame t + shift of y reads, zeros in front of the signal included
        assert torch.equal(b[..., shift:shift + a.shape[-1] - 1].view(torch.int32), a[..., :-1].view(torch.int32)), shift


def test_a_batch_is_its_planes_run_alone():
    import torch

    import alac.net_amd as pkg

    spec = pkg.ConstantQ(SR, hop_length=48, f_min=FMIN, n_bins=21, log="ln")
    x = torch.from_numpy(np.stack([signal(2, 1700, 6), signal(2, 1700, 7), signal(2, 1700, 8)])).cuda()        # [3, 2, T]
    whole, lens = pkg.cqt(x, spec, lengths=[1700, 5, -1])
    assert whole.shape == (3, 2, 21, 1 + 1700 // 48) and lens.tolist() == [36, 1, -1]
    for b in range(3):
        for c in range(2):
            assert torch.equal(pkg.cqt(x[b, c], spec).view(torch.int32), whole[b, c].view(torch.int32))


def test_what_is_not_finite_stays_in_its_support_and_is_never_hidden():
    import torch

    import alac.net_amd as pkg

    spec = pkg.ConstantQ(SR, hop_length=50, f_min=FMIN, n_bins=30)
    N = pkg.cqt_lengths(spec)
    x = signal(2, 50 * 70, 9)                                           # 71 frames: three tiles
    clean = pkg.cqt(torch.from_numpy(x).cuda(), spec).cpu().numpy()
    t = np.arange(clean.shape[-1])
    first = t[None, :] * 50 - (N // 2)[:, None]
    for i, v in ((1700, np.nan), (0, np.inf), (50 * 70 - 1, -np.inf), (50 * 33 - N[0] // 2, np.nan)):
        y = x.copy()
        y[0, i] = v
        got = pkg.cqt(torch.from_numpy(y).cuda(), spec).cpu().numpy()
        twin = pkg.cqt_host_f32(y, spec)
        reached = (first <= i) & (i < first + N[:, None])
        assert reached.any() and not np.isfinite(got[0][reached]).any(), i
        assert np.array_equal(np.isnan(got), np.isnan(twin)), i
        # a NaN's payload and sign are the one exception to bit for bit: every other element is the twin's
        ok = ~np.isnan(twin)
        assert np.array_equal(got[ok].view(np.int32), twin[ok].view(np.int32)), i
        assert np.array_equal(got[0][~reached].view(np.int32), clean[0][~reached].view(np.int32)), i
        assert np.array_equal(got[1].view(np.int32), clean[1].view(np.int32)), i
        assert (reached.any(axis=0) & ~reached.all(axis=0)).any()      # per bin: a frame holds both kinds


def test_an_empty_batch_launches_nothing_and_the_refusals():
    import torch

    import alac.net_amd as pkg

    spec = pkg.ConstantQ(SR, hop_length=64, f_min=FMIN, n_bins=30)
    out = pkg.cqt(torch.empty((0, 2, 500), device="cuda"), spec)
    assert out.shape == (0, 2, 30, 8)
    out, lens = pkg.cqt(torch.empty((0, 500), device="cuda"), spec, lengths=[])
    assert out.shape == (0, 30, 8) and lens.shape == (0,)
    for bad in (torch.zeros(500), torch.zeros(500, device="cuda", dtype=torch.float64), torch.zeros((2, 0), device="cuda")):
        with pytest.raises(ValueError):
            pkg.cqt(bad, spec)
    with pytest.raises(ValueError):
        pkg.cqt(torch.zeros(500, device="cuda"), pkg.LogMel(16000))
    # the C ABI refuses what the table cannot be: lengths that rise, a frame count that is not the row's
    x = torch.zeros((1, 1, 500), device="cuda")
    table, lens = spec.device_tables(x.device)
    o = torch.empty((1, 1, 30, 8), device="cuda")
    with pkg.AlacGpuContext([(512, 16, 40, 10, 14, 2)]) as ctx:
        ctx.cqt_device(x, 1, 1, 500, 500, 64, 30, spec.lens, lens, table, 1, 0, 1e-10, o, 8)
        rising = np.array(spec.lens)
        rising[3] = rising[2] + 1
        for args in ((64, 30, rising, 1, 0, 1e-10, 8), (64, 30, spec.lens, 3, 0, 1e-10, 8), (64, 30, spec.lens, 1, 3, 1e-10, 8),
                     (64, 30, spec.lens, 1, 0, 0.0, 8), (64, 30, spec.lens, 1, 0, 1e-10, 7), (0, 30, spec.lens, 1, 0, 1e-10, 8)):
            hop, nb, ln, pw, lm, fl, of = args
            with pytest.raises(pkg.AlacGpuError):
                ctx.cqt_device(x, 1, 1, 500, 500, hop, nb, ln, lens, table, pw, lm, fl, o, of)
    torch.cuda.synchronize()
