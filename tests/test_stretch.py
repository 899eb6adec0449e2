"""alacgpu_time_stretch_device and the pitch shift built on it against their float32 twins (alac.net_amd/pitch.py), bit for bit,
on the smallest shapes that reach every path: rows outside the corpus (-1), empty, too short to reflect (256), the smallest
live row (257: three STFT frames), lengths that are and are not multiples of the hop, every factor of the issue's list and 1
in one batch, one and two channels, the three transform sizes (512 and 2048 lead with a radix-2 stage, 1024 does not), a
plane stride above the frames and a source one float off 16-byte alignment.  NaNs stand behind every row's length and all over
the rows that are left alone: nothing there is read, nothing there is written."""
from fractions import Fraction as F

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, STRIDE, RATE = 1400, 1416, 16000
FACTORS = (F(1, 2), F(2), F(9, 10), F(11, 10), F(200, 189), F(1))
# (channels, n_fft, lengths, the factors' rotation, layout)
CASES = {
    "c1-512-short": (1, 512, (-1, 0, 256, 257, 384, 1000), 3, "stride"),
    "c2-512-short": (2, 512, (-1, 0, 256, 257, 384, 1000), 2, "offset"),
    "c1-512-long": (1, 512, (1153, 1280, 1000, 257, 384, 1400), 0, "offset"),
    "c2-512-long": (2, 512, (1153, 1280, 1000, 257, 384, 1400), 0, "stride"),
    "c2-1024": (2, 1024, (512, 513, 1153, 1280, 1400, 1000), 1, "stride"),
    "c1-2048": (1, 2048, (1024, 1025, 1153, 1280, 1400, 1200), 4, "offset"),
}
_cache = {}


def case(name):
    """(x float32 [6, C, T] with NaNs behind the lengths, factors, lengths, n_fft, layout), the same arrays every time"""
    if name not in _cache:
        C, n_fft, lengths, turn, layout = CASES[name]
        rng = np.random.default_rng(sorted(CASES).index(name))
        x = (0.25 * rng.standard_normal((6, C, T))).astype(np.float32)
        x += (0.5 * np.sin(2 * np.pi * 440.0 / RATE * np.arange(T))).astype(np.float32)
        factors = [FACTORS[(b + turn) % 6] for b in range(6)]
        for b, v in enumerate(lengths):
            x[b, :, max(v, 0):] = np.nan
        _cache[name] = (x, factors, np.asarray(lengths, dtype=np.int64), n_fft, layout)
    return _cache[name]


def twin(name, what):
    import alac.net_amd as pkg

    key = (name, what)
    if key not in _cache:
        x, factors, lengths, n_fft, _ = case(name)
        _cache[key] = (pkg.time_stretch_host_f32(x, factors, lengths, n_fft) if what == "stretch"
                       else pkg.pitch_shift_host_f32(x, factors, RATE, lengths, n_fft))
    return _cache[key]


def on_device(torch, x, layout):
    """x as a device tensor that is the slice [..., :T] of planes of STRIDE frames; "offset": one float off 16-byte alignment"""
    B, C, _ = x.shape
    flat = torch.full((B * C * STRIDE + 4,), float("nan"), dtype=torch.float32, device="cuda")
    d = flat[1 if layout == "offset" else 0:][:B * C * STRIDE].view(B, C, STRIDE)[..., :T]
    assert (d.data_ptr() % 16 == 4) == (layout == "offset")
    d.copy_(torch.from_numpy(x))
    return d


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def is_live(v, f, n_fft):
    return f != 1 and v > n_fft // 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_time_stretch_equals_its_twin_bit_for_bit(name):
    import torch

    import alac.net_amd as pkg

    x, factors, lengths, n_fft, layout = case(name)
    want, want_lengths = twin(name, "stretch")
    d = on_device(torch, x, layout)
    y, new_lengths = pkg.time_stretch(d, factors, lengths, n_fft)
    again, _ = pkg.time_stretch(d, factors, torch.from_numpy(lengths).cuda(), n_fft)
    v = np.clip(lengths, 0, T)
    spec = [(2 * int(v[b]) * f.numerator + f.denominator) // (2 * f.denominator) if is_live(int(v[b]), f, n_fft) else int(v[b])
            for b, f in enumerate(factors)]
    assert new_lengths.cpu().tolist() == spec == want_lengths.tolist()
    assert y.shape == want.shape and np.array_equal(bits(y), bits(want))
    assert np.array_equal(bits(again), bits(y))
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("name", ["c2-512-short", "c1-2048"])
def test_the_entry_point_leaves_rows_alone_and_writes_the_lengths(name):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import _context

    x, factors, lengths, n_fft, layout = case(name)
    want, want_lengths = twin(name, "stretch")
    d = on_device(torch, x, layout)
    B, C, _ = x.shape
    Lo = want.shape[2]
    out = torch.full((B, C, Lo + 8), float("nan"), dtype=torch.float32, device="cuda")
    d_p = torch.tensor([f.numerator for f in factors], dtype=torch.int32, device="cuda")
    d_q = torch.tensor([f.denominator for f in factors], dtype=torch.int32, device="cuda")
    d_new = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    _context(0).time_stretch_device(d, out, B, C, STRIDE, Lo + 8, T, Lo, d_p, d_q, torch.from_numpy(lengths).cuda(), d_new, n_fft,
                                    stream=torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    kept = [int(min(lengths[b], T)) for b in range(B)]
    for b, f in enumerate(factors):
        if is_live(int(lengths[b]), f, n_fft):
            assert int(d_new[b]) == int(want_lengths[b])
            assert np.array_equal(bits(got[b, :, :Lo]), bits(want[b])), b          # zeros behind the new length, up to out_frames
        else:
            assert int(d_new[b]) == kept[b]                                       # -1 stays -1
            assert np.isnan(got[b, :, :Lo]).all(), b
    assert np.isnan(got[:, :, Lo:]).all()                                          # behind out_frames


@pytest.mark.parametrize("name", sorted(CASES))
def test_pitch_shift_equals_its_twin_in_place_and_out_of_place(name):
    import torch

    import alac.net_amd as pkg

    x, factors, lengths, n_fft, layout = case(name)
    x = x.copy()
    for b, f in enumerate(factors):             # the rows that are left alone: NaNs all over
        if not is_live(int(lengths[b]), f, n_fft):
            x[b] = np.nan
    want = pkg.pitch_shift_host_f32(x, factors, RATE, lengths, n_fft)
    d = on_device(torch, x, layout)
    y = pkg.pitch_shift(d, factors, RATE, lengths, n_fft)
    assert y is not d and np.array_equal(bits(d), bits(x))
    assert np.array_equal(bits(y), bits(want))
    for b, f in enumerate(factors):
        v = int(np.clip(lengths[b], 0, T))
        assert np.isnan(want[b, :, v:]).all()
        if is_live(v, f, n_fft):
            assert np.isfinite(want[b, :, :v]).all(), b
    same = pkg.pitch_shift(d, factors, RATE, torch.from_numpy(lengths).cuda(), n_fft, out=d)
    assert same is d and np.array_equal(bits(d), bits(want))


@pytest.mark.parametrize("name", ["c2-512-long", "c2-1024"])
def test_pitch_shift_is_the_stretch_and_the_speed_perturbation(name):
    import torch

    import alac.net_amd as pkg

    x, factors, lengths, n_fft, layout = case(name)
    d = on_device(torch, x, layout)
    y = pkg.pitch_shift(d, factors, RATE, lengths, n_fft)
    s, ls = pkg.time_stretch(d, factors, lengths, n_fft)
    r, lr = pkg.speed_perturb(s, factors, RATE, RATE, lengths=ls)
    got, r = y.cpu().numpy(), r.cpu().numpy()
    for b, f in enumerate(factors):
        v = int(np.clip(lengths[b], 0, T))
        if not is_live(v, f, n_fft):
            assert np.array_equal(bits(got[b]), bits(x[b]))
            continue
        assert abs(int(lr[b]) - v) <= 2                                            # the duration is kept
        n = min(v, r.shape[2])
        assert np.array_equal(bits(got[b, :, :n]), bits(r[b, :, :n])) and not got[b, :, n:v].any()
        assert np.isnan(got[b, :, v:]).all()


def test_refusals():
    import torch

    import alac.net_amd as pkg

    x = torch.zeros((2, 1, 600), dtype=torch.float32, device="cuda")
    for bad in (lambda: pkg.time_stretch(x.cpu(), 1.1), lambda: pkg.time_stretch(x, [1.1]), lambda: pkg.time_stretch(x, 3),
                lambda: pkg.time_stretch(x, 1.1, n_fft=256), lambda: pkg.time_stretch(x, 1.1, lengths=[1.0, 2.0]),
                lambda: pkg.pitch_shift(x, 1.1, 16000.0), lambda: pkg.pitch_shift(x, 1.1, 16000, out=x[:, :, :300]),
                lambda: pkg.pitch_shift(torch.zeros((2, 3, 600), device="cuda"), 1.1, 16000),
                lambda: pkg.pitch_shift(x.to(torch.float64), 1.1, 16000), lambda: pkg.pitch_shift(x, F(1, 3), 16000)):
        with pytest.raises(ValueError):
            bad()
    y, n = pkg.time_stretch(x[:0], [])
    assert y.shape == (0, 1, 0) and n.shape == (0,)
