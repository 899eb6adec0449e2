"""alacgpu_pyin_device on the GPU, bit for bit its float32 twin in numpy (pyin.pyin_host_f32) on all three lines, on the
smallest shapes that reach each path of csrc/alac_pyin.hip; then the two stages alone -- `pyin_observation` against the twin's
observations, `pyin_decode` against the twin's recursion on hand-built observations -- and the arguments of `alac.pyin`.

As in tests/test_yin.py every call goes through `run`: the input is the slice [..., :T] of a tensor whose slack behind every
plane is NaN, the output may lie between guards; the guards, the input's bytes and the absence of a NaN in the track are
checked after every call."""
import numpy as np
import pytest

from test_yin_spec import same_bits, voiced_noise

pytestmark = pytest.mark.gpu

SLACK = 7
GUARD = 64


def small(**kw):
    """49 bins, h = 8 at 8 kHz: the cheapest spec that has everything"""
    import alac.net_amd as pkg

    return pkg.PYin(8000, 64, 80, 200.0, 800.0, **{"resolution": 0.5, **kw})


def specs():
    import alac.net_amd as pkg

    return {"small": small(), "default": pkg.PYin(16000), "h0": small(max_transition_rate=1.0), "wide": small(max_transition_rate=500.0),
            "switch": small(switch_prob=0.5), "one": small(n_thresholds=1), "many": small(n_thresholds=256),
            "kaldi": small(center=False, align_length=100), "odd_hop": pkg.PYin(8000, 64, 81, 200.0, 800.0, resolution=0.5)}


def test_the_grid_is_what_it_says():
    s = specs()
    assert (s["small"].n_bins, s["small"].h) == (49, 8) and (s["default"].n_bins, s["default"].h) == (329, 40)
    assert s["h0"].h == 0 and s["wide"].h >= s["wide"].n_bins and s["wide"].band == 48 and s["odd_hop"].hop_length % 4


def run(torch, pkg, x, spec, lengths=None, slack=SLACK, give_out=False):
    B, C, T = x.shape
    src = np.full((B, C, T + slack), np.nan, dtype=np.float32)
    src[..., :T] = x
    d_src = torch.from_numpy(src).cuda()
    view = d_src[..., :T] if slack else d_src
    n = int(spec.frames(T))
    out = None
    if give_out:
        raw = torch.full((B * C * 3 * n + 2 * GUARD,), 12345.0, dtype=torch.float32, device="cuda")
        out = raw[GUARD:GUARD + B * C * 3 * n].view(B, C, 3, n)
    got = pkg.pyin(view, spec, lengths, out=out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, C, 3, n) and got.dtype == torch.float32
    if give_out:
        assert got.data_ptr() == out.data_ptr()
        assert bool((torch.cat([raw[:GUARD], raw[GUARD + B * C * 3 * n:]]) == 12345.0).all()), "a guard was written"
    assert np.array_equal(d_src.cpu().numpy(), src, equal_nan=True), "the samples were written"
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), "the track is not finite"
    return got


def check(torch, pkg, x, spec, lengths=None, **kw):
    got = run(torch, pkg, x, spec, lengths, **kw)
    want = pkg.pyin_host_f32(x, spec, lengths)
    assert same_bits(got, want), (spec, np.argwhere(got.view(np.int32) != want.view(np.int32))[:5])
    if lengths is not None:
        for b, n in enumerate(spec.lengths(np.clip(np.asarray(lengths), 0, x.shape[-1]))):
            assert not got[b, :, :, n:].any()
    return got


def sine_and_silence(B, C, T, rate):
    t = np.arange(T) / rate
    x = np.stack([0.5 * np.sin(2 * np.pi * (220.0 + 40.0 * k) * t) for k in range(B * C)]).reshape(B, C, T)
    x[..., T // 3:T // 2] = 0.0
    return x.astype(np.float32)


@pytest.mark.parametrize("name", ["small", "default", "h0", "wide", "switch", "one", "many", "kaldi", "odd_hop"])
def test_the_kernels_are_the_twin_bit_for_bit(name):
    """[3, 2, 2000] of tones in noise with the lengths 0, 37 and T, then whole rows into a guarded `out`"""
    import torch

    import alac.net_amd as pkg

    spec = specs()[name]
    x = voiced_noise(3, 2, 2000, spec.sample_rate, seed=len(name))
    got = check(torch, pkg, x, spec, [0, 37, 2000])
    assert got[2, :, 1].any(), "no voiced frame: the test shows little"
    check(torch, pkg, x, spec, None, give_out=True)


def test_lengths_at_the_edges_and_two_dimensions():
    """Lengths 0, shorter than one frame, exactly one frame (T' = 1: no transition), full, beyond T and -1, centred and not;
    [B, T] is [B, 1, T]"""
    import torch

    import alac.net_amd as pkg

    kaldi, centred = specs()["kaldi"], specs()["small"]
    x = voiced_noise(6, 1, 2000, 8000, seed=3)
    lengths = [0, 99, 100, 2000, 2500, -1]
    assert list(kaldi.lengths(np.asarray(lengths))) == [0, 0, 1, 24, 31, -1]
    got = check(torch, pkg, x, kaldi, lengths)
    assert not got[0].any() and not got[1].any() and not got[5].any() and got[2, 0, 0, 0] > 0 and not got[2, :, :, 1:].any()
    check(torch, pkg, x, centred, [0, 1, 79, 80, 2000, -1])
    flat = torch.from_numpy(x[:2, 0]).cuda()
    got2 = pkg.pyin(flat, centred).cpu().numpy()
    assert got2.shape == (2, 3, 26) and same_bits(got2, pkg.pyin_host_f32(x[:2, 0], centred))


@pytest.mark.parametrize("name", ["small", "default"])
def test_signals(name):
    """Noise alone, a sine with a stretch of silence, all silence -- every unvoiced state ties on every frame, so the tie rule
    alone picks the path: the first unvoiced state --, and a row with one NaN and one with one infinity"""
    import torch

    import alac.net_amd as pkg

    spec = specs()[name]
    rate, T = spec.sample_rate, 2000
    rng = np.random.default_rng(11)
    check(torch, pkg, (0.3 * rng.standard_normal((2, 1, T))).astype(np.float32), spec)
    check(torch, pkg, sine_and_silence(1, 2, T, rate), spec)
    got = check(torch, pkg, np.zeros((1, 2, T), dtype=np.float32), spec)
    assert not got[:, :, 1:].any() and (got[:, :, 0] == spec.tables()["freq"][0]).all()
    x = voiced_noise(2, 1, T, rate, seed=5)
    x[0, 0, 700], x[1, 0, 900] = np.nan, np.inf
    src = torch.from_numpy(x).cuda()
    got = pkg.pyin(src, spec).cpu().numpy()
    assert np.isfinite(got).all() and same_bits(got, pkg.pyin_host_f32(x, spec))


@pytest.mark.parametrize("name", ["small", "default", "kaldi"])
def test_the_observation_alone_is_the_twins(name):
    import torch

    import alac.net_amd as pkg

    spec = specs()[name]
    x = np.concatenate([voiced_noise(2, 2, 2000, spec.sample_rate, seed=9), sine_and_silence(1, 2, 2000, spec.sample_rate)])
    lengths = [2000, 1234, 2000]
    _, info = pkg.pyin_host_f32(x, spec, lengths, details=True)
    got = [g.cpu().numpy() for g in pkg.pyin_observation(torch.from_numpy(x).cuda(), spec, lengths)]
    for g, key in zip(got, ("obs_voiced", "obs_unvoiced", "vp")):
        assert same_bits(g, info[key]), (key, np.argwhere(g.view(np.int32) != info[key].view(np.int32))[:5])
    assert (got[0][0, 0, :5] > -126).any() and (got[0][0] == -126).any()


def decode_both(torch, pkg, ov, ou, spec, counts=None):
    from alac.net_amd.pyin import pyin_decode_host

    got = pkg.pyin_decode(torch.from_numpy(ov).cuda(), torch.from_numpy(ou).cuda(), spec, counts)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = pyin_decode_host(ov, ou, spec, counts, f32=True)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    return got


@pytest.mark.parametrize("name", ["small", "default", "h0", "wide", "switch"])
def test_the_decode_alone_on_hand_built_observations(name):
    import torch

    import alac.net_amd as pkg

    spec = specs()[name]
    n, h, F = spec.n_bins, spec.h, 12
    # all equal: ties everywhere, the lowest source state wins every one of them
    got = decode_both(torch, pkg, np.full((1, 2, F, n), -3.0, dtype=np.float32), np.full((1, 2, F), -3.0, dtype=np.float32), spec)
    assert got.min() >= 0
    # one sharp ridge that jumps by more than h bins between two frames (where the band leaves room for such a jump)
    ov = np.full((2, 1, F, n), -126.0, dtype=np.float32)
    ridge = np.where(np.arange(F) < F // 2, 3, min(n - 2, 3 + h + 5))
    ov[:, 0, np.arange(F), ridge] = -0.5
    ou = np.full((2, 1, F), -20.0, dtype=np.float32)
    got = decode_both(torch, pkg, ov, ou, spec, [F, 7])
    assert (got[1, 0, 7:] == -1).all() and (got[1, 0, :3] == 3).all()
    # vp = 1 on every frame: the unvoiced states at the floor
    rng = np.random.default_rng(n)
    ov = np.log2(rng.uniform(0.01, 1.0, (1, 2, F, n))).astype(np.float32)
    got = decode_both(torch, pkg, ov, np.full((1, 2, F), -126.0, dtype=np.float32), spec)
    assert (got < n).all()
    # frame counts 0 and 1
    got = decode_both(torch, pkg, ov, np.full((1, 2, F), -126.0, dtype=np.float32), spec, [0])
    assert (got == -1).all()
    decode_both(torch, pkg, ov, np.full((1, 2, F), -5.0, dtype=np.float32), spec, [1])


def test_a_long_walk_back():
    """700 frames of 49 bins: a ridge that wanders by up to h bins a frame over noise, so the path wanders with it and the walk
    back is 700 dependent loads through many states"""
    import torch

    import alac.net_amd as pkg

    spec = small()
    rng = np.random.default_rng(700)
    ov = np.log2(rng.uniform(1e-6, 1e-3, (2, 1, 700, 49))).astype(np.float32)
    ridge = np.abs((24 + np.cumsum(rng.integers(-8, 9, (2, 700)), axis=1)) % 96 - 48) % 49
    for r in range(2):
        ov[r, 0, np.arange(700), ridge[r]] = -0.25
    ou = np.log2(rng.uniform(1e-3, 1e-2, (2, 1, 700))).astype(np.float32)
    got = decode_both(torch, pkg, ov, ou, spec, [700, 699])
    assert len(np.unique(got[0])) > 10


def test_arguments():
    import torch

    import alac.net_amd as pkg

    spec = small()
    x = torch.from_numpy(voiced_noise(2, 2, 2000, 8000, seed=1)).cuda()
    n = int(spec.frames(2000))
    with pytest.raises(ValueError, match="PYin"):
        pkg.pyin(x, pkg.Yin(8000, 64, 80, 200.0, 800.0))
    with pytest.raises(ValueError, match="PYin"):
        pkg.pyin_observation(x, pkg.Yin(8000, 64, 80, 200.0, 800.0))
    for bad in (torch.empty((2, 2, 2, n), device="cuda"), torch.empty((2, 2, 3, n + 1), device="cuda"),
                torch.empty((2, 2, 3, n), device="cuda", dtype=torch.float64), torch.empty((2, 2, 3, 2 * n), device="cuda")[..., ::2]):
        with pytest.raises(ValueError, match="out must be"):
            pkg.pyin(x, spec, out=bad)
    wide = torch.zeros(2 * 2 * 2000 + 2 * 2 * 3 * n, device="cuda")
    pcm = wide[:8000].view(2, 2, 2000)
    with pytest.raises(ValueError, match="overlaps"):
        pkg.pyin(pcm, spec, out=wide[7000:7000 + 12 * n].view(2, 2, 3, n))
    with pytest.raises(ValueError):
        pkg.pyin(x, spec, lengths=[1, 2, 3])
    with pytest.raises(ValueError):
        pkg.pyin(x.cpu(), spec)
    with pytest.raises(ValueError, match="2\\^31"):
        pkg.pyin(torch.empty((1 << 12, 1, 1600), device="cuda"), pkg.PYin(16000, hop_length=1))     # 4096 lines of 1601 frames
    ov = torch.zeros((1, 1, 5, 49), device="cuda")
    with pytest.raises(ValueError, match="obs_voiced"):
        pkg.pyin_decode(ov[..., :48], torch.zeros((1, 1, 5), device="cuda"), spec)
    with pytest.raises(ValueError, match="obs_voiced"):
        pkg.pyin_decode(ov, torch.zeros((1, 1, 4), device="cuda"), spec)
    with pytest.raises(ValueError):
        pkg.pyin_decode(ov, torch.zeros((1, 1, 5), device="cuda"), spec, frame_counts=[1, 2])
