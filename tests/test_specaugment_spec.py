"""The host side of SpecAugment (alac.net_amd/augment.py), without a device: what SpecAugment refuses, the signatures and the
C ABI entry, the draws on CPU tensors against their bounds, and the float32 twin against hand-computed values, its exact
cases and the bound of the module docstring, |twin - float64| <= 8 * 2^-24 * max(|x[i]|, |x[i + 1]|)."""
import inspect
import os
import re

import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
U = 2.0 ** -24


def test_specaugment_refuses_what_it_should_and_is_immutable():
    import alac.net_amd as pkg

    a = pkg.SpecAugment()
    assert (a.freq_masks, a.freq_width, a.time_masks, a.time_width, a.time_ratio, a.time_warp, a.fill, a.p) == (2, 27, 2, 100, 1.0, 0, 0.0, 1.0)
    b = pkg.SpecAugment(1, 15, 3, 50, 0.2, 5, -1.5, 0.5)
    assert b == pkg.SpecAugment(freq_masks=1, freq_width=15, time_masks=3, time_width=50, time_ratio=0.2, time_warp=5, fill=-1.5, p=0.5)
    assert hash(b) == hash(pkg.SpecAugment(1, 15, 3, 50, 0.2, 5, -1.5, 0.5)) and a != b and a == pkg.SpecAugment() and len({a, b}) == 2
    assert pkg.SpecAugment(0, 0, 0, 0, 0.0, 0, 3, 0).p == 0.0 and "time_warp=5" in repr(b)
    for name in ("freq_masks", "freq_width", "time_masks", "time_width", "time_warp"):
        for bad in (-1, 1.0, 2.5, "2", None, True, NAN):
            with pytest.raises(ValueError):
                pkg.SpecAugment(**{name: bad})
    for name in ("time_ratio", "p"):
        for bad in (-0.1, 1.5, NAN, INF, "1", None, True):
            with pytest.raises(ValueError):
                pkg.SpecAugment(**{name: bad})
    for bad in (NAN, INF, -INF, 1e39, "0", None, True):
        with pytest.raises(ValueError):
            pkg.SpecAugment(fill=bad)
    for name in a.__slots__:
        with pytest.raises(AttributeError):
            setattr(a, name, 1)
        with pytest.raises(AttributeError):
            delattr(a, name)
    with pytest.raises(AttributeError):
        a.other = 1


def test_crops_take_augment_in_front_of_sample_rate_and_mono():
    import alac.net_amd as pkg

    for fn in (pkg.Corpus.crops, pkg.Corpus.random_crops):
        p = inspect.signature(fn).parameters
        assert p["augment"].default is None
        assert list(p)[-3:] == ["augment", "sample_rate", "mono"]
    assert pkg.spec_augment and pkg.specaugment_host and pkg.specaugment_host_f32 and pkg.SpecAugment


def test_specaugment_entry_is_declared_bound_and_refuses_null():
    import alac.net_amd as pkg

    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+alacgpu_specaugment_device\s*\(([^)]*)\)", src)
    assert m, "include/alacgpu.h does not declare alacgpu_specaugment_device"
    assert len(m.group(1).split(",")) == len(pkg.SYMBOLS["alacgpu_specaugment_device"][1]) == 16
    assert hasattr(pkg.lib(), "alacgpu_specaugment_device")
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    assert "alacgpu_specaugment_device(" in cs
    # a NULL ctx is refused before anything touches a device
    assert pkg.lib().alacgpu_specaugment_device(None, None, None, 1, 1, 1, 4, 4, None, None, None, 0, None, 0, 0.0, None) == -1


def test_the_header_and_the_module_agree():
    import importlib

    au = importlib.import_module("alac.net_amd.augment")
    assert au.WAVE_MAX == header_constant("ALAC_AUG_WAVE_MAX", "alac_augment.h")
    assert au.LDS_MAX == header_constant("ALAC_AUG_LDS_MAX", "alac_augment.h") >= 16384
    assert au.MAX_MASKS == header_constant("ALAC_AUG_MAX_MASKS", "alac_augment.h")
    for bad in (dict(freq_masks=au.MAX_MASKS + 1), dict(time_masks=au.MAX_MASKS + 1)):
        with pytest.raises(ValueError):
            au.SpecAugment(**bad)


# ---- the draws -----------------------------------------------------------------------------------------------------------------
M, N, B, W = 80, 120, 512, 5


def lengths_cpu(torch):
    lens = torch.randint(0, N + 1, (B,), generator=torch.Generator().manual_seed(1))
    lens[:7] = torch.tensor([-1, 0, 1, 2 * W + 2, 2 * W + 3, N, 3])
    return lens


def test_every_draw_lies_within_its_bounds():
    import torch

    import alac.net_amd as pkg

    lens = lengths_cpu(torch)
    tau = lens.clamp(min=0)
    spec = pkg.SpecAugment(freq_masks=2, freq_width=27, time_masks=3, time_width=40, time_ratio=0.5, time_warp=W, p=0.8)
    warp, freq, time = spec.draw(M, lens, generator=torch.Generator().manual_seed(2))
    assert warp.shape == (B, 2) and freq.shape == (B, 2, 2) and time.shape == (B, 3, 2)
    assert warp.dtype == freq.dtype == time.dtype == torch.int32 and warp.device == lens.device
    f0, fw, t0, tw = freq[..., 0], freq[..., 1], time[..., 0], time[..., 1]
    assert bool(((f0 >= 0) & (fw >= 0) & (fw <= 27) & (f0 + fw <= M)).all())
    assert bool(((t0 >= 0) & (tw >= 0) & (t0 + tw <= tau[:, None])).all())
    assert bool((tw <= torch.minimum(torch.tensor(40), tau // 2)[:, None]).all())
    c, c1 = warp[:, 0].long(), warp[:, 1].long()
    on = c != 0
    assert bool((on == (c1 != 0)).all()) and bool((tau[on] > 2 * W + 2).all()) and not bool(on[3]) and not bool(on[:3].any())
    assert bool(((c[on] >= 1) & (c1[on] >= 1) & (c[on] <= tau[on] - 2) & (c1[on] <= tau[on] - 2) & ((c1[on] - c[on]).abs() <= W)).all())
    assert bool(((c[on] >= W + 1) & (c[on] <= tau[on] - 2 - W)).all())
    # a crop is kept or not as a whole; one without frames gets nothing; p = 0.8 of the 500 or so with frames
    nothing = (warp == 0).all(1) & (freq == 0).all(2).all(1) & (time == 0).all(2).all(1)
    assert bool(nothing[tau == 0].all()) and 40 <= int(nothing[tau > 0].sum()) <= 170
    kept = ~nothing
    assert bool(on[kept & (tau > 2 * W + 2)].all())              # every kept crop that is long enough is warped (c >= W + 1 > 0)
    # the row of 2 W + 3 frames has one place for c
    again = pkg.SpecAugment(time_warp=W).draw(M, lens, generator=torch.Generator().manual_seed(3))[0]
    assert again[4, 0] == W + 1 and abs(int(again[4, 1]) - (W + 1)) <= W
    # each extreme occurs: a width of 0 and the largest, the first and the last start, both ends of the shift
    assert bool((fw[kept] == 0).any()) and bool((fw[kept] == 27).any()) and bool((tw[kept] == 0).any())
    assert bool((tw[kept] == torch.minimum(torch.tensor(40), tau // 2)[kept][:, None]).any()) and bool((tw == 40).any())
    assert bool((f0[kept] == 0).any()) and bool(((f0 + fw == M) & (fw > 0)).any()) and bool(((t0 + tw == tau[:, None]) & (tw > 0)).any())
    assert bool(((c1 - c)[on] == W).any()) and bool(((c1 - c)[on] == -W).any()) and bool(((c1 - c)[on] == 0).any())


def test_draws_follow_the_seed_and_their_number_does_not_follow_the_parameters(monkeypatch):
    import torch

    import alac.net_amd as pkg

    lens = lengths_cpu(torch)
    spec = pkg.SpecAugment(time_warp=W, p=0.5)
    a = spec.draw(M, lens, generator=torch.Generator().manual_seed(4))
    b = spec.draw(M, lens, generator=torch.Generator().manual_seed(4))
    c = spec.draw(M, lens, generator=torch.Generator().manual_seed(5))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(x, y) for x, y in zip(a, c))
    none = pkg.SpecAugment(time_warp=W, p=0.0).draw(M, lens, generator=torch.Generator().manual_seed(4))
    assert all(not bool(t.any()) for t in none)
    assert pkg.SpecAugment(0, 27, 0, 100).draw(M, lens)[1].shape == (B, 0, 2)
    # 3 + 2 freq_masks + 2 time_masks calls of rand, B float64 values each, whatever the other parameters are -- and the
    # generator is left where any other policy of those counts leaves it
    calls = []
    rand = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, **kw: calls.append((a, kw.get("dtype"))) or rand(*a, **kw))
    states = set()
    for kw in (dict(), dict(time_warp=W), dict(p=0.0), dict(p=0.3, time_warp=50, time_ratio=0.0), dict(freq_width=0, time_width=0),
               dict(fill=2.0, freq_width=10 ** 6, time_width=10 ** 6)):
        g = torch.Generator().manual_seed(6)
        del calls[:]
        pkg.SpecAugment(freq_masks=2, time_masks=3, **kw).draw(M, lens, generator=g)
        assert len(calls) == 3 + 2 * 2 + 2 * 3 and all(c == ((B,), torch.float64) for c in calls), kw
        states.add(bytes(g.get_state().tolist()))
    assert len(states) == 1
    with pytest.raises(ValueError):
        spec.draw(M, lens.double())
    with pytest.raises(ValueError):
        spec.draw(-1, lens)
    with pytest.raises(ValueError):
        spec.draw(M, lens.tolist())


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def pairs(*rows):
    return np.array(rows, dtype=np.int32)


def test_the_twin_on_cases_whose_answer_is_known():
    from alac.net_amd.augment import _source, specaugment_host, specaugment_host_f32

    rng = np.random.default_rng(10)
    x = rng.standard_normal((3, 2, 5, 31)).astype(np.float32)
    for fn in (specaugment_host_f32, specaugment_host):
        # no draws, draws of zeros, and a warp with c == c': the identity, bit for bit
        assert same_bits(fn(x).astype(np.float32), x) and same_bits(fn(x, lengths=[31, 0, -1]).astype(np.float32), x)
        assert same_bits(fn(x, np.zeros((3, 2), np.int32), np.zeros((3, 2, 2), np.int32), np.zeros((3, 1, 2), np.int32)).astype(np.float32), x)
        assert same_bits(fn(x, pairs((7, 7), (1, 1), (29, 29))).astype(np.float32), x)
        # a pair outside 1 .. tau - 2 is no warp
        assert same_bits(fn(x, pairs((0, 3), (3, 0), (30, 4)), lengths=[31, 31, 31]).astype(np.float32), x)
        assert same_bits(fn(x, pairs((3, 4), (3, 4), (2, 1)), lengths=[5, 4, 3]).astype(np.float32)[1:], x[1:])
    # by hand on 7 frames, c = 2 -> c' = 4: s = 0, 1/2, 1, 3/2, 2 | 2 + (t - 4) 4 / 2 = 4, 6
    h = np.array([[[[1.0, 3.0, 4.0, 8.0, 16.0, 32.0, 64.0]]]], dtype=np.float32)
    want = np.array([1.0, 2.0, 3.0, 3.5, 4.0, 16.0, 64.0], dtype=np.float32)
    assert same_bits(specaugment_host_f32(h, pairs((2, 4)))[0, 0, 0], want) and np.array_equal(specaugment_host(h, pairs((2, 4)))[0, 0, 0], want)
    # ... and c = 4 -> c' = 2: s = 0, 2, 4 | 4 + (t - 2) 2 / 4 = 4.5, 5, 5.5, 6
    want = np.array([1.0, 4.0, 16.0, 24.0, 32.0, 48.0, 64.0], dtype=np.float32)
    assert same_bits(specaugment_host_f32(h, pairs((4, 2)))[0, 0, 0], want)
    # the same warp over the first 7 of 9 frames: the two behind stay
    h9 = np.concatenate([h, np.array([[[[NAN, INF]]]], dtype=np.float32)], axis=3)
    got = specaugment_host_f32(h9, pairs((4, 2)), lengths=[7])[0, 0, 0]
    assert same_bits(got[:7], want) and same_bits(got[7:], h9[0, 0, 0, 7:])
    # the ends and frame c' are copies, the source index does not decrease, and x[i + 1] is not read where r == 0
    for tau, c, c1 in ((31, 10, 15), (31, 15, 10), (31, 1, 29), (31, 29, 1), (3, 1, 1), (4, 1, 2), (4, 2, 1), (16384, 8000, 8005)):
        i, r, den = _source(tau, c, c1)
        assert i[0] == 0 and r[0] == 0 and i[c1] == c and r[c1] == 0 and i[-1] == tau - 1 and r[-1] == 0
        assert (np.diff(i) >= 0).all() and (r >= 0).all() and (r < den).all() and (den >= 1).all() and ((i + 1 <= tau - 1) | (r == 0)).all()
    y = specaugment_host_f32(x, pairs((10, 15), (15, 10), (1, 29)))
    for b, c1, c in ((0, 15, 10), (1, 10, 15), (2, 29, 1)):
        assert same_bits(y[b, ..., 0], x[b, ..., 0]) and same_bits(y[b, ..., 30], x[b, ..., 30]) and same_bits(y[b, ..., c1], x[b, ..., c])
        assert not same_bits(y[b], x[b])
    z = x.copy()
    z[0, :, :, 11] = INF                                       # frame c' = 15 reads x[10] with r == 0: the infinity next to it stays out
    y = specaugment_host_f32(z, pairs((10, 15), (0, 0), (0, 0)))
    assert same_bits(y[0, ..., 15], x[0, ..., 10]) and np.isfinite(y[0, ..., :15]).all() and not np.isfinite(y[0, ..., 16]).any()
    z[0, :, :, 30] = NAN
    assert same_bits(specaugment_host_f32(z, pairs((10, 15), (0, 0), (0, 0)), lengths=[30, 31, 31])[0, ..., 29], z[0, ..., 29])


def test_masks_override_the_warp_and_nothing_behind_tau_is_touched():
    from alac.net_amd.augment import specaugment_host, specaugment_host_f32

    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 2, 6, 40)).astype(np.float32)
    x[:, :, :, 33:] = NAN
    warp = pairs((12, 9), (0, 0))
    freq = np.array([[(1, 2), (2, 1), (5, 4)], [(0, 0), (3, 0), (-1, 2)]], dtype=np.int32)
    time = np.array([[(0, 3), (30, 10)], [(5, 5), (8, 4)]], dtype=np.int32)
    lens = [33, 20]
    plain = specaugment_host_f32(x, warp, lengths=lens)
    y = specaugment_host_f32(x, warp, freq, time, lens, fill=-2.5)
    m = np.zeros(x.shape, dtype=bool)
    m[0, :, 1:3, :33] = m[0, :, 5:, :33] = m[0, :, :, 0:3] = m[0, :, :, 30:33] = True
    m[1, :, 0:1, :20] = m[1, :, :, 5:12] = True
    assert (y[m] == -2.5).all() and same_bits(y[~m], plain[~m]) and m[0].sum() and m[1].sum()
    assert same_bits(y[0, ..., 33:], x[0, ..., 33:]) and same_bits(y[1, ..., 20:], x[1, ..., 20:])
    y64, dY = specaugment_host(x, warp, freq, time, lens, fill=-2.5, bound=True)
    assert (y64[m] == -2.5).all() and (dY[m] == 0).all() and (dY[1] == 0).all() and (dY[0, :, 0, 3:30] > 0).any()
    for bad in (dict(warp=np.zeros((3, 2), np.int32)), dict(freq=np.zeros((2, 2), np.int32)), dict(time=np.zeros((2, 1, 3), np.int32)),
                dict(warp=np.zeros((2, 2), np.float32)), dict(lengths=[1]), dict(fill=NAN)):
        with pytest.raises(ValueError):
            specaugment_host_f32(x, **bad)
    with pytest.raises(ValueError):
        specaugment_host_f32(x.astype(np.float64))
    with pytest.raises(ValueError):
        specaugment_host_f32(x[0])


def test_the_twin_stays_within_the_bound_of_the_float64_statement():
    from alac.net_amd.augment import specaugment_host, specaugment_host_f32

    rng = np.random.default_rng(12)
    worst = 0.0
    for tau, c, c1 in ((201, 100, 105), (201, 50, 45), (97, 1, 95), (97, 95, 1), (3000, 1500, 1495), (16384, 8000, 8005)):
        x = (rng.standard_normal((1, 2, 3, tau + 2)) * 2.0 ** rng.integers(-20, 21, (1, 2, 3, tau + 2))).astype(np.float32)
        y64, dY = specaugment_host(x, pairs((c, c1)), lengths=[tau], bound=True)
        y32 = specaugment_host_f32(x, pairs((c, c1)), lengths=[tau])
        err = np.abs(y32.astype(np.float64) - y64)
        assert (err <= dY).all(), (tau, c, c1, float((err - dY).max()))
        assert (dY[..., tau:] == 0).all() and same_bits(y32[..., tau:], x[..., tau:])
        worst = max(worst, float((err[dY > 0] / dY[dY > 0]).max()))
    print(f"max |twin - float64| / bound = {worst:.3f}")
    assert worst > 0.01              # (the bound is not vacuous: the twin uses a visible part of it)
