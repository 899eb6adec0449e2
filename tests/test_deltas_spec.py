"""deltas.py without a device: Kaldi's delta filters, the specification `deltas_host` on ramps and at the edges -- where Kaldi's
clamp into the ORIGINAL features differs from a replicate-padded first-order delta applied twice --, the lengths, and the
float32 twin against the specification."""
import numpy as np
import pytest

U = 2.0 ** -24


def replicate_delta(x, W):
    """One first-order delta with replicate padding over the last axis (what a padded conv1d per order computes)"""
    T = x.shape[-1]
    idx = np.clip(np.arange(T)[:, None] + np.arange(-W, W + 1)[None, :], 0, T - 1)
    return (x[..., idx] * (np.arange(-W, W + 1) / (2.0 * sum(j * j for j in range(1, W + 1))))).sum(axis=-1)


def test_scales():
    import alac.net_amd as pkg

    s1, s2 = pkg.delta_scales(2, 2)
    first = np.array([-2, -1, 0, 1, 2]) / 10.0
    assert s1.dtype == np.float32 and np.array_equal(s1, first.astype(np.float32))
    assert np.array_equal(s2, np.convolve(first, first).astype(np.float32)) and s2.shape == (9,)
    assert np.allclose(s2, [0.04, 0.04, 0.01, -0.04, -0.1, -0.04, 0.01, 0.04, 0.04], atol=1e-7)
    assert [len(s) for s in pkg.delta_scales(3, 4)] == [9, 17, 25]
    assert np.array_equal(pkg.delta_scales(1, 1)[0], np.array([-0.5, 0, 0.5], dtype=np.float32))
    spec = pkg.Deltas()
    assert (spec.order, spec.window) == (2, 2) and spec.lines(13) == 39 and spec == pkg.Deltas(2, 2) and spec != pkg.Deltas(1, 2)
    assert np.array_equal(spec.scales, np.concatenate([s1, s2])) and not spec.scales.flags.writeable
    with pytest.raises(AttributeError):
        spec.order = 1
    for bad in (dict(order=0), dict(order=4), dict(window=0), dict(window=5), dict(order=True), dict(order=2.0)):
        with pytest.raises(ValueError):
            pkg.Deltas(**bad)


def test_a_ramp_and_its_edges():
    import alac.net_amd as pkg

    spec = pkg.Deltas(2, 2)
    ramp = (3.0 * np.arange(40) + 1.0).astype(np.float32).reshape(1, 1, 1, 40)
    out = pkg.deltas_host(ramp, spec)
    assert out.shape == (1, 1, 3, 40) and out.dtype == np.float64
    assert np.array_equal(out[0, 0, 0], ramp[0, 0, 0])
    assert np.abs(out[0, 0, 1, 2:-2] - 3.0).max() <= 1e-6            # the slope, where no clamp acts
    assert np.abs(out[0, 0, 2, 4:-4]).max() <= 1e-6                  # order 2 of a ramp is 0 there
    # six frames 0 .. 5: Kaldi's order 2 at the edges, computed by hand from the nine scales and clamp(t + j, 0, 5)
    six = np.arange(6, dtype=np.float32).reshape(1, 1, 1, 6)
    got = pkg.deltas_host(six, spec)[0, 0]
    assert np.abs(got[1] - [0.5, 0.8, 1.0, 1.0, 0.8, 0.5]).max() <= 1e-6
    kaldi = np.array([0.26, 0.21, 0.08, -0.08, -0.21, -0.26])
    assert np.abs(got[2] - kaldi).max() <= 1e-6
    twice = replicate_delta(replicate_delta(six[0, 0].astype(np.float64), 2), 2)[0]
    assert np.abs(twice - [0.13, 0.15, 0.08, -0.08, -0.15, -0.13]).max() <= 1e-12
    assert (np.abs(got[2] - twice)[[0, 1, 4, 5]] > 0.05).all()       # not "delta applied twice with replicate padding"
    # in the interior of a longer signal the two agree
    x = np.random.default_rng(0).standard_normal((1, 1, 2, 30)).astype(np.float32)
    k, r = pkg.deltas_host(x, spec)[0, 0, 4:6], replicate_delta(replicate_delta(x[0, 0].astype(np.float64), 2), 2)
    assert np.abs(k - r)[:, 4:-4].max() <= 1e-6 and np.abs(k - r)[:, :2].max() > 1e-3


def test_lengths():
    import alac.net_amd as pkg

    rng = np.random.default_rng(1)
    x = rng.standard_normal((6, 2, 3, 11)).astype(np.float32)
    for order, W in ((2, 2), (3, 1), (2, 4)):
        spec = pkg.Deltas(order, W)
        lens = [1, 2, W, 11, 0, -1]
        out, d = pkg.deltas_host(x, spec, lengths=lens, bound=True)
        twin = pkg.deltas_host_f32(x, spec, lengths=lens)
        assert out.shape == (6, 2, 3 * (order + 1), 11) and twin.dtype == np.float32
        assert np.array_equal(out[:, :, :3], x) and np.array_equal(twin[:, :, :3], x)       # the static block, whatever len
        # len 1: every clamp collapses on frame 0, whose delta is x[0] times the sum of the rounded scales
        assert np.abs(out[0, :, 3:]).max() <= 1e-6 and np.abs(twin[0, :, 3:]).max() <= 1e-6
        for b, n in enumerate(lens):
            n = max(n, 0)
            assert (out[b, :, 3:, n:] == 0).all() and (twin[b, :, 3:, n:] == 0).all()      # behind len, and rows of len <= 0
            if n:
                assert np.array_equal(out[b, :, :, :n], pkg.deltas_host(x[b:b + 1, ..., :n], spec)[0])     # nothing behind len is read
        assert out[1, :, 3:6, :2].any() and out[3, :, 3:].any()
        err = np.abs(twin.astype(np.float64) - out)
        assert (err <= d).all() and (d[:, :, :3] == 0).all()
        assert np.array_equal(pkg.deltas_host(x, spec, lengths=[11] * 6), pkg.deltas_host(x, spec))
        assert np.array_equal(pkg.deltas_host(x, spec, lengths=[99] * 6), pkg.deltas_host(x, spec))
    # a NaN behind len reaches no delta
    y = x.copy()
    y[3, :, :, 7:] = np.nan
    a, b = pkg.deltas_host_f32(y, pkg.Deltas(), lengths=[11, 11, 11, 7, 11, 11]), pkg.deltas_host_f32(x, pkg.Deltas(), lengths=[11, 11, 11, 7, 11, 11])
    assert np.array_equal(a[:, :, 3:], b[:, :, 3:]) and np.isnan(a[3, :, :3, 7:]).all()
    for bad in (lambda: pkg.deltas_host(x[0], pkg.Deltas()), lambda: pkg.deltas_host(x.astype(np.float64), pkg.Deltas()),
                lambda: pkg.deltas_host(x, 2), lambda: pkg.deltas_host(x, pkg.Deltas(), lengths=[1, 2]),
                lambda: pkg.deltas_host_f32(x, pkg.Deltas(), lengths=np.ones(6))):
        with pytest.raises(ValueError):
            bad()


def test_the_twin_against_the_specification():
    import alac.net_amd as pkg

    x = (np.random.default_rng(2).standard_normal((2, 1, 13, 50)) * 20).astype(np.float32)
    for order, W in ((1, 2), (2, 2), (3, 1), (2, 4), (3, 4)):
        spec = pkg.Deltas(order, W)
        out, d = pkg.deltas_host(x, spec, bound=True)
        err = np.abs(pkg.deltas_host_f32(x, spec).astype(np.float64) - out)
        assert (err <= d).all() and err.max() > 0
        for k in range(1, order + 1):                                  # the bound is (2 k W + 2) u sum |scales x|
            taps = np.abs(x[0, 0, 0, 20 - k * W:20 + k * W + 1].astype(np.float64) * pkg.delta_scales(order, W)[k - 1])
            assert abs(d[0, 0, 13 * k, 20] - (2 * k * W + 2) * U * taps.sum()) <= 1e-18
