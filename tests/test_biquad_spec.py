"""alac.net_amd/biquad.py without a device: the cookbook designers against scipy's Butterworth designs and their own defining
properties, the sequential specification against scipy.signal.sosfilt, the blocked twin against the specification within the
derived bound D -- on random sections and on the two filters that float32 cannot do, a 20 Hz high-pass and a 20 Hz low-pass
of Q 10 at 48 kHz --, the identity rows, the lengths, and the `Effects` policy's draws."""
import sys

import numpy as np
import pytest

import alac.net_amd as pkg

bq = sys.modules["alac.net_amd.biquad"]
U32 = 2.0 ** -24


def response(q, w):
    """H(e^jw) of sections q [..., S, 5] at the angles w [n]: the product over the sections"""
    z = np.exp(-1j * np.asarray(w))
    q = np.asarray(q)[..., None]
    h = (q[..., 0, :] + q[..., 1, :] * z + q[..., 2, :] * z * z) / (1.0 + q[..., 3, :] * z + q[..., 4, :] * z * z)
    return h.prod(axis=-2)


def noise(shape, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def stable_sections(rng, shape):
    """Random stable sections: poles of radius up to 0.98, any numerator"""
    r, th = rng.uniform(0.1, 0.98, shape), rng.uniform(0.05, 3.0, shape)
    q = rng.uniform(-1.0, 1.0, shape + (5,))
    q[..., 3], q[..., 4] = -2.0 * r * np.cos(th), r * r
    return q


HARD = (("highpass", 20.0, 0.707), ("lowpass", 20.0, 10.0))


# ---- the designers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,btype", [("lowpass", "low"), ("highpass", "high")])
def test_the_second_order_butterworth(kind, btype):
    signal = pytest.importorskip("scipy.signal")
    for fs, f in ((16000.0, 300.0), (48000.0, 20.0), (44100.0, 9000.0), (8000.0, 3400.0)):
        b, a = signal.butter(2, f, btype=btype, fs=fs)
        got = pkg.__dict__[kind](fs, f, 1.0 / np.sqrt(2.0))
        want = np.concatenate([b / a[0], a[1:] / a[0]])
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (kind, fs, f, got, want)


def test_telephone_is_the_fourth_order_butterworth_band():
    signal = pytest.importorskip("scipy.signal")
    import torch

    fs = 16000.0
    q, g = pkg.Effects.telephone().draw(1, fs, generator=torch.Generator().manual_seed(0))
    assert q.shape == (1, 4, 5) and float(g[0]) == 1.0
    w = np.pi * (np.arange(64) + 0.5) / 64
    want = np.ones(64, dtype=complex)
    for f, btype in ((300.0, "high"), (3400.0, "low")):
        want = want * signal.sosfreqz(signal.butter(4, f, btype=btype, fs=fs, output="sos"), worN=w)[1]
    assert np.abs(response(q.numpy()[0], w) - want).max() <= 1e-10


def test_what_the_designs_promise():
    fs = 44100.0
    f = np.array([100.0, 1000.0, 5000.0, 15000.0])
    for db in (-9.0, 4.0):
        at = np.abs(response(pkg.peaking(fs, f, 2.0, db)[:, None, :], 2 * np.pi * f / fs))
        assert np.allclose(20 * np.log10(np.diagonal(at)), db, atol=1e-9)
        assert np.allclose(20 * np.log10(np.abs(response(pkg.lowshelf(fs, f, 0.7, db)[:, None, :], [0.0]))), db, atol=1e-9)
        assert np.allclose(20 * np.log10(np.abs(response(pkg.highshelf(fs, f, 0.7, db)[:, None, :], [np.pi]))), db, atol=1e-9)
    w = np.linspace(0.01, 3.1, 50)
    assert np.allclose(np.abs(response(pkg.allpass(fs, f, 0.5)[:, None, :], w)), 1.0, atol=1e-12)
    assert np.allclose(np.abs(np.diagonal(response(pkg.bandpass(fs, f, 3.0)[:, None, :], 2 * np.pi * f / fs))), 1.0, atol=1e-12)
    # (the zero: a numerator of three terms of size 2 rounded to 2^-52 each, over a denominator of about 2 alpha = 5e-4 at 100 Hz)
    assert np.abs(np.diagonal(response(pkg.bandreject(fs, f, 3.0)[:, None, :], 2 * np.pi * f / fs))).max() <= 1e-11
    assert pkg.lowpass(fs, f).shape == (4, 5) and pkg.lowpass(fs, 100.0).shape == (5,)


@pytest.mark.parametrize("args", [(16000, 0.0), (16000, 8000.0), (16000, 9000.0), (16000, -5.0), (16000, 100.0, 0.0),
                                  (16000, 100.0, -1.0), (16000, float("nan")), (16000, 100.0, float("inf")),
                                  (16000, 100.0, 0.7, float("nan")), (float("inf"), 100.0)])
def test_the_designers_refuse(args):
    for fn in (pkg.lowpass, pkg.highpass, pkg.bandpass, pkg.bandreject, pkg.allpass, pkg.peaking, pkg.lowshelf, pkg.highshelf):
        with pytest.raises(ValueError):
            fn(*args)


def test_the_policy_refuses():
    for bad in (lambda: pkg.RandomBiquad("notch", 100.0), lambda: pkg.RandomBiquad("lowpass", 0.0),
                lambda: pkg.RandomBiquad("lowpass", (200.0, 100.0)), lambda: pkg.RandomBiquad("lowpass", 100.0, q=0.0),
                lambda: pkg.RandomBiquad("lowpass", 100.0, p=1.5), lambda: pkg.Effects(gain=(0.5, 2), gain_db=(-6, 6)),
                lambda: pkg.Effects(filters=("lowpass",)), lambda: pkg.Effects(p=-0.1),
                lambda: pkg.Effects((pkg.RandomBiquad("lowpass", 100.0),) * 9), lambda: pkg.Effects(clamp=1)):
        with pytest.raises(ValueError):
            bad()
    fx = pkg.Effects((pkg.RandomBiquad("lowpass", (100.0, 8000.0)),))
    with pytest.raises(ValueError):
        fx.draw(4, 16000)
    with pytest.raises(AttributeError):
        fx.p = 0.5
    assert fx == pkg.Effects((pkg.RandomBiquad("lowpass", (100.0, 8000.0)),)) and hash(fx) == hash(pkg.Effects(fx.filters))


# ---- the specification and the twin ----------------------------------------------------------------------------------------------
def test_the_specification_is_sosfilt():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    x = noise((3, 2, 700), 1)
    q = stable_sections(rng, (3, 4))
    g = np.array([0.5, -2.0, 1.0])
    s, D = pkg.biquad_host(x, q, gain=g, bound="sequential")
    assert np.all(D <= pkg.biquad_host(x, q, gain=g, bound=True)[1]) and D.max() > 0
    for b in range(3):
        sos = np.concatenate([q[b, :, :3], np.ones((4, 1)), q[b, :, 3:]], axis=1)
        want = g[b] * signal.sosfilt(sos, x[b].astype(np.float64), axis=-1)
        # (both are sequential float64 evaluations of the same cascade, sosfilt's in the transposed form: 8 rounded quantities
        # a sample, each an addition to a later output: the sequential share of the bound alone, none of the blocked one)
        assert np.all(np.abs(s[b] - want) <= D[b]), (b, np.abs(s[b] - want).max(), D[b].max())


def test_the_twin_is_within_the_bound_on_random_sections():
    rng = np.random.default_rng(6)
    for T in (1, 2, 17, bq.TILE + 5):
        x = noise((4, 2, T), T)
        q = stable_sections(rng, (4, 3))
        g = rng.uniform(0.125, 2.0, 4)
        s, D = pkg.biquad_host(x, q, gain=g, bound=True)
        y = pkg.biquad_host_twin(x, q, gain=g)
        assert y.dtype == np.float32 and np.all(np.abs(y - s) <= U32 * np.abs(s) + D), T


def test_the_twin_is_within_the_bound_on_the_two_hard_filters():
    x = noise((2, 1, 32000), 0)
    q = np.stack([pkg.__dict__[kind](48000.0, f, qq)[None] for kind, f, qq in HARD])
    s, D = pkg.biquad_host(x, q, bound=True)
    y = pkg.biquad_host_twin(x, q)
    r = np.stack([bq._twin_rows(x[b].astype(np.float64), q[b:b + 1], np.ones(1)) for b in range(2)])
    print("blocked float64 against sequential:", np.abs(r - s).max(axis=(1, 2)), "D:", D.max(axis=(1, 2)),
          "float32 results that differ:", (y != s.astype(np.float32)).sum(axis=(1, 2)))
    assert np.all(np.abs(r - s) <= D) and np.all(np.abs(y - s) <= U32 * np.abs(s) + D)
    # D is above the peak on these rows and says nothing.  What the number formats promise does: a row is float32, rounded
    # once, so the float64 evaluation stays below one float32 rounding of the row's peak (biquad.py's docstring)
    peak = np.abs(s).max(axis=(1, 2), keepdims=True)
    assert np.all(np.abs(r - s) <= U32 * peak), (np.abs(r - s).max(axis=(1, 2)), U32 * peak.ravel())
    assert np.all(np.abs(y - s) <= U32 * np.abs(s) + U32 * peak)


def test_identity_rows_and_lengths():
    x = noise((6, 2, 40), 3)
    q = np.tile(np.array(bq.IDENTITY), (6, 2, 1))
    q[1:, 0] = pkg.lowpass(16000.0, 1000.0)
    lengths = np.array([40, -1, 0, 1, 2, 40])
    for fn in (pkg.biquad_host, pkg.biquad_host_twin):
        y = fn(x, q, lengths)
        assert np.array_equal(y[:3].astype(np.float32), x[:3])                 # identity, -1 and 0: as they are
        for b in (3, 4):
            assert np.array_equal(y[b, :, lengths[b]:].astype(np.float32), x[b, :, lengths[b]:])
            assert not np.array_equal(y[b, :, :lengths[b]].astype(np.float32), x[b, :, :lengths[b]])
        whole = fn(x[5:], q[5:])
        assert np.array_equal(y[5], whole[0])
        # a shorter length is the same filter on fewer frames
        assert np.array_equal(y[4, :, :2], fn(x[4:5, :, :2], q[4:5])[0])
    # a gain alone, and the clamp, make a row live
    g = np.array([2.0, 1, 1, 1, 1, 1])
    assert np.array_equal(pkg.biquad_host_twin(x, q, gain=g)[0], 2 * x[0])
    big = (x * 20).astype(np.float32)
    big[0, 0, 5] = np.nan
    c = pkg.biquad_host_twin(big, q, clamp=True)
    assert np.isnan(c[0, 0, 5]) and np.nanmax(np.abs(c)) <= 1.0 and np.array_equal(c[0, 1], np.clip(big[0, 1], -1, 1))
    for bad in (lambda: pkg.biquad_host(x.astype(np.float64), q), lambda: pkg.biquad_host(x, q[:, :, :4]),
                lambda: pkg.biquad_host(x, np.zeros((6, 9, 5))), lambda: pkg.biquad_host(x, q, gain=np.ones(5)),
                lambda: pkg.biquad_host(x, q, lengths=np.ones(6))):
        with pytest.raises(ValueError):
            bad()


def test_draws_are_reproducible_and_keep_their_shares():
    import torch

    fx = pkg.Effects((pkg.RandomBiquad("peaking", (100.0, 4000.0), q=(0.5, 2.0), gain_db=(-6.0, 6.0), p=0.25),
                      pkg.RandomBiquad("highpass", 40.0)), gain=(0.125, 2.0), p=0.5)
    B = 4096
    q, g = fx.draw(B, 16000, generator=torch.Generator().manual_seed(7))
    q2, g2 = fx.draw(B, 16000, generator=torch.Generator().manual_seed(7))
    assert q.dtype == torch.float64 and q.shape == (B, 2, 5) and g.dtype == torch.float64 and g.shape == (B,)
    assert torch.equal(q, q2) and torch.equal(g, g2)
    ident = torch.tensor(bq.IDENTITY, dtype=torch.float64)
    off = (q == ident).all(dim=2)                           # [B, 2]: the section is the identity
    crop_off = off[:, 1]                                    # the high-pass is always drawn: off only with the crop
    assert torch.all(g[crop_off] == 1.0) and torch.all(off[crop_off, 0])
    # the shares, within five standard deviations of a binomial
    for share, p in ((float((~crop_off).double().mean()), 0.5), (float((~off[~crop_off, 0]).double().mean()), 0.25)):
        assert abs(share - p) <= 5 * np.sqrt(p * (1 - p) / (B * 0.4)), (share, p)
    live = g[~crop_off]
    assert 0.125 <= float(live.min()) and float(live.max()) <= 2.0 and 0.9 < float(live.mean()) < 1.2
    # the drawn sections are the designer's
    hp = torch.from_numpy(pkg.highpass(16000.0, 40.0, 0.7071))
    assert torch.allclose(q[~crop_off, 1], hp.expand(int((~crop_off).sum()), 5), rtol=1e-12, atol=0)
    # the same number of draws whatever the arguments: a generator is left where another policy of two filters leaves it
    ga, gb = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    fx.draw(8, 16000, generator=ga)
    pkg.Effects((pkg.RandomBiquad("lowpass", 100.0), pkg.RandomBiquad("lowpass", 200.0))).draw(8, 16000, generator=gb)
    assert torch.equal(torch.rand(4, generator=ga), torch.rand(4, generator=gb))
    # decibels, and nothing at all
    q, g = pkg.Effects(gain_db=(-6.0, -6.0)).draw(3, 8000, generator=torch.Generator().manual_seed(0))
    assert q.shape == (3, 1, 5) and torch.all(q == ident) and torch.allclose(g, torch.full((3,), 10 ** -0.3, dtype=torch.float64))
