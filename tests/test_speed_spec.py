"""speed.py without a device: factors and ratios, the float32 weights against the table's within EPS_W, the float32 twin
against the float64 specification within the stated bound, and the draws."""
import math
from fractions import Fraction

import numpy as np
import pytest

RATIOS = [(9, 10), (11, 10), (10, 9), (3969, 1600), (441, 160), (33, 5)]


def random_ratios(n=50, below=4000, seed=2024):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        a, b = (int(v) for v in rng.integers(1, below, 2))
        if math.gcd(a, b) == 1 and (a, b) not in out:
            out.append((a, b))
    return out


ALL = RATIOS + random_ratios()


def signal(rate, frames, seed):
    """The stereo signal of tests/test_corpus_mixed_rates.py, float32 [2, frames]"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / rate
    x = np.stack([0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + c) + 0.01 * rng.standard_normal(frames) for c in (0, 1)])
    return x.astype(np.float32)


def test_factors_and_their_refusals():
    from alac.net_amd.speed import SpeedPerturb, _factor

    assert _factor(0.9) == Fraction(9, 10) and _factor(1.1) == Fraction(11, 10) and _factor(1) == 1 and _factor(np.float64(0.95)) == Fraction(19, 20)
    assert _factor(Fraction(7, 8)) == Fraction(7, 8) and _factor(2) == 2 and _factor(0.5) == Fraction(1, 2)
    for bad in (0.49, 2.01, 3, Fraction(1001, 1002), 0.90001, float("nan"), "0.9", None, True):
        with pytest.raises(ValueError):
            _factor(bad)
    sp = SpeedPerturb()
    assert sp.factors == (Fraction(9, 10), Fraction(1), Fraction(11, 10)) and sp.one == 1 and sp.p == 1.0
    assert SpeedPerturb((0.9, 1.1)).factors == (Fraction(9, 10), Fraction(11, 10), Fraction(1)) and SpeedPerturb((0.9, 1.1)).one == 2
    assert SpeedPerturb((0.9, 1.1)).weights == (1.0, 1.0, 0.0)
    for kw in (dict(factors=()), dict(factors=(0.9, Fraction(9, 10))), dict(factors=(0.9, 3.0)), dict(p=1.5), dict(p=-0.1),
               dict(weights=(1, 2)), dict(weights=(0, 0, 0)), dict(weights=(1, -1, 1)), dict(factors=0.9)):
        with pytest.raises(ValueError):
            SpeedPerturb(**kw)
    with pytest.raises(AttributeError):
        sp.p = 0.5
    assert sp == SpeedPerturb((0.9, 1, 1.1)) and hash(sp) == hash(SpeedPerturb((0.9, 1, 1.1))) and sp != SpeedPerturb((0.9, 1.1))


def test_ratio_and_frames():
    from alac.net_amd.resample import filter_width, resampled_frames
    from alac.net_amd.speed import ratio

    assert ratio(44100, 0.9, 16000) == (3969, 1600, 16)
    assert ratio(16000, Fraction(11, 10), 16000)[:2] == (11, 10)
    assert ratio(48000, 1.1, 8000)[:2] == (33, 5)
    for r in (8000, 16000, 44100):
        assert ratio(r, 1, r)[:2] == (1, 1)
    for rate, f, new in ((44100, 0.9, 16000), (48000, 1.1, 8000), (22050, 1.1, 16000), (16000, 0.9, 16000)):
        a, b, width = ratio(rate, f, new)
        assert math.gcd(a, b) == 1 and Fraction(a, b) == Fraction(rate, new) * Fraction(repr(f)) and width == filter_width(a, b)
        for T in (0, 1, 2999, 20000):
            assert resampled_frames(T, a, b) == -(-b * T // a) == int(resampled_frames(np.array([T]), a, b)[0])
    with pytest.raises(ValueError):
        ratio(0, 1, 16000)
    with pytest.raises(ValueError):
        ratio(16000, 3, 16000)


@pytest.mark.parametrize("a,b", RATIOS)
def test_source_window_covers_every_tap(a, b):
    from alac.net_amd.resample import filter_width, resampled_frames, source_window

    width, L = filter_width(a, b), 1500
    Ty = resampled_frames(20000, a, b)
    for o in (0, b - 1, b, Ty - 1):
        s0, Ls = source_window(o, L, a, b, width)
        j = o + np.arange(L, dtype=np.int64)
        lo, hi = (j * a) // b - width, (j * a) // b + width
        assert lo.min() >= s0 and hi.max() < s0 + Ls, (a, b, o)


def test_weights_are_within_eps_w_of_the_table():
    """max |w32 - w64| / scale over every phase and tap of every ratio: under EPS_W, which is derived, not measured"""
    from alac.net_amd.resample import _table, filter_width
    from alac.net_amd.speed import EPS_W, weights_f32

    assert EPS_W == 2.0 ** -18
    worst = 0.0
    for a, b in ALL:
        width = filter_width(a, b)
        d0, w64 = _table(a, b, width)
        phases = (np.arange(b, dtype=np.int64) * a) % b
        assert np.array_equal(d0, (np.arange(b, dtype=np.int64) * a) // b - width)
        w32 = weights_f32(a, b, width, phases)
        assert w32.dtype == np.float32 and w32.shape == w64.shape and np.isfinite(w32).all()
        scale = 0.99 * min(a, b) / a
        e = float(np.abs(w32.astype(np.float64) - w64.astype(np.float64)).max()) / scale
        assert e <= EPS_W, (a, b, e)
        worst = max(worst, e)
    print(f"worst |w32 - w64| / scale over {len(ALL)} ratios: {worst:.3e} = {worst * 2 ** 24:.2f} * 2^-24; EPS_W {EPS_W:.3e}")


def test_fma32_is_exact():
    from alac.net_amd.speed import _fma32

    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(2000).astype(np.float32), rng.standard_normal(2000).astype(np.float32)
    z = (rng.standard_normal(2000) * 10.0 ** rng.integers(-6, 3, 2000)).astype(np.float32)
    # a case that rounding twice gets wrong: the product's tail decides a tie of the float64 sum
    x = np.concatenate([x, np.float32([1 + 2.0 ** -12])])
    y = np.concatenate([y, np.float32([1 + 2.0 ** -12])])
    z = np.concatenate([z, np.float32([2.0 ** 29])])
    got = _fma32(x, y, z)
    for i in range(len(x)):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        g = np.float32(got[i])
        near = [np.nextafter(g, np.float32(-np.inf)), g, np.nextafter(g, np.float32(np.inf))]
        d = [abs(Fraction(float(v)) - exact) for v in near]
        assert d[1] <= d[0] and d[1] <= d[2], i
        if d[1] == d[0] or d[1] == d[2]:        # a tie: to even
            assert (g.view(np.uint32) & 1) == 0, i


@pytest.mark.parametrize("mono", [False, True])
def test_twin_is_within_the_bound_of_the_specification(mono):
    from alac.net_amd.resample import filter_width
    from alac.net_amd.speed import speed_bound, speed_host, speed_host_f32

    x = signal(44100, 3000, 50)
    worst = 0.0
    for a, b in ALL:
        width = filter_width(a, b)
        want = speed_host(x.astype(np.float64), a, b, width, mono=mono)
        tol = speed_bound(x.astype(np.float64), a, b, width, mono=mono)
        got = speed_host_f32(x, a, b, width, mono=mono)
        assert got.dtype == np.float32 and got.shape == want.shape == (1 if mono else 2, -(-b * 3000 // a))
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= tol).all(), (a, b, float((err / np.maximum(tol, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print(f"mono={mono}: worst err / bound {worst:.3f}")


def test_twin_windows_and_edges():
    """origin, first and num_frames: a window of the twin is the whole signal's frames, bit for bit, and zero outside it"""
    from alac.net_amd.speed import speed_host_f32

    x = signal(44100, 3000, 51)
    for a, b, width in ((3969, 1600, 16), (11, 10, 7)):
        whole = speed_host_f32(x, a, b, width)
        Ty = whole.shape[1]
        part = speed_host_f32(x, a, b, width, first=-5, num_frames=Ty + 20)
        assert not part[:, :5].any() and not part[:, 5 + Ty:].any()
        assert np.array_equal(part[:, 5:5 + Ty].view(np.uint32), whole.view(np.uint32))
        cut = speed_host_f32(x[:, 100:2000], a, b, width, origin=100, first=300, num_frames=200)
        full = speed_host_f32(np.concatenate([np.zeros((2, 100), np.float32), x[:, 100:2000]], axis=1), a, b, width, first=300, num_frames=200)
        assert np.array_equal(cut.view(np.uint32), full.view(np.uint32))


def test_draws():
    import torch

    from alac.net_amd.speed import SpeedPerturb

    g = lambda: torch.Generator().manual_seed(7)
    sp = SpeedPerturb()
    k = sp.draw(4096, generator=g(), device="cpu")
    assert k.dtype == torch.int64 and k.shape == (4096,) and int(k.min()) == 0 and int(k.max()) == 2
    assert torch.equal(k, sp.draw(4096, generator=g(), device="cpu"))
    assert all(1100 < int((k == i).sum()) < 1650 for i in range(3))
    assert (SpeedPerturb(p=0.0).draw(512, generator=g(), device="cpu") == 1).all()
    two = SpeedPerturb((0.9, 1.1))
    k2 = two.draw(4096, generator=g(), device="cpu")
    assert int(k2.max()) == 1 and int(k2.min()) == 0                     # the appended factor 1 has weight 0 ...
    k3 = SpeedPerturb((0.9, 1.1), p=0.5).draw(4096, generator=g(), device="cpu")
    assert set(k3.tolist()) == {0, 1, 2} and 1800 < int((k3 == 2).sum()) < 2300      # ... and is what 1 - p gives
    assert torch.equal(torch.where(k3 == 2, k2, k3), k2)
    kw = SpeedPerturb((0.9, 1.0, 1.1), weights=(0, 0, 1)).draw(256, generator=g(), device="cpu")
    assert (kw == 2).all()


def test_the_table_path_still_refuses_a_large_table():
    from alac.net_amd.resample import resample_table

    with pytest.raises(ValueError):
        resample_table(39690, 16000)
