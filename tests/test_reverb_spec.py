"""The host side of the reverberation (alac.net_amd/reverb.py): Reverb, the float64 specification against what it must give
on responses whose answer is known and against scipy, the float32 twin against the derived bound dY on every shape of the
grid of tests/test_reverb.py, the rows that stay, and NaN containment.  CPU only, except the draws, which need the device.

dY bounds every float32 evaluation in the kernel's scheme, so the twin has r = max |twin - specification| / dY <= 1; the tests
on the GPU hold the kernel to r_gpu <= 4 r_twin."""
import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import noise, same_bits

INF, NAN = float("inf"), float("nan")
N = header_constant("ALAC_REVERB_N", "alac_reverb.h")
H = N // 2


class _Open:
    """What stands in for an alacgpu context in a Corpus that never saw a device"""

    def close(self):
        pass


@pytest.fixture
def hollow():
    """A Corpus object without a device behind it: open as far as Reverb looks"""
    import alac.net_amd as pkg

    c = pkg.Corpus.__new__(pkg.Corpus)
    c._gpu, c._pinned, c.channels = _Open(), None, 1
    yield c
    c._gpu = None


def test_reverb_refuses_what_it_cannot_draw_and_is_immutable(hollow):
    import alac.net_amd as pkg

    a = pkg.Reverb(hollow)
    assert a.rirs is hollow and a.p == 1.0 and a.max_seconds == 1.0 and a.frames(16000) == 16000 and a.frames(44100) == 44100
    b = pkg.Reverb(hollow, p=0.25, max_seconds=0.5)
    assert b.p == 0.25 and b.frames(16000) == 8000 and b == pkg.Reverb(hollow, 0.25, 0.5) and hash(b) == hash(pkg.Reverb(hollow, 0.25, 0.5))
    assert a != b and pkg.Reverb(hollow, p=0).p == 0.0 and pkg.Reverb(hollow, max_seconds=1e-9).frames(16000) == 1
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=NAN), dict(p="1"), dict(p=None), dict(p=True), dict(max_seconds=0), dict(max_seconds=-1.0),
                dict(max_seconds=NAN), dict(max_seconds=INF), dict(max_seconds="1"), dict(max_seconds=None), dict(max_seconds=1e39)):
        with pytest.raises(ValueError):
            pkg.Reverb(hollow, **bad)
    for bad in (None, "rirs", 3, object()):
        with pytest.raises(ValueError):
            pkg.Reverb(bad)
    for name, value in (("p", 0.5), ("max_seconds", 2.0), ("rirs", None)):
        with pytest.raises(AttributeError):
            setattr(a, name, value)
        with pytest.raises(AttributeError):
            delattr(a, name)
    with pytest.raises(AttributeError):
        a.other = 1
    hollow.channels = 3
    with pytest.raises(ValueError):
        pkg.Reverb(hollow)
    hollow.channels = 2
    pkg.Reverb(hollow)
    hollow._gpu = None                      # closed
    with pytest.raises(ValueError):
        pkg.Reverb(hollow)
    with pytest.raises(ValueError):
        a.draw(4)


def test_the_header_and_the_module_agree():
    import importlib

    rv = importlib.import_module("alac.net_amd.reverb")       # (the package's `reverb` is the function)
    assert rv.N == N and rv.HOP == H and rv.THREADS == header_constant("ALAC_REVERB_THREADS", "alac_reverb.h")
    assert rv.STAGES == header_constant("ALAC_REVERB_STAGES", "alac_reverb.h") and 4 ** rv.STAGES == N
    c, s = rv.twiddles()
    k = np.arange(N)
    assert c.dtype == s.dtype == np.float32 and c[0] == 1 and s[0] == 0 and c[N // 4] == np.float32(np.cos(np.pi / 2)) and s[N // 4] == -1
    assert np.abs(c.astype(np.float64) - np.cos(2 * np.pi * k / N)).max() <= 2.0 ** -24 * 1.001
    assert np.abs(s.astype(np.float64) + np.sin(2 * np.pi * k / N)).max() <= 2.0 ** -24 * 1.001


def test_one_tap_is_the_signal_itself_with_the_taps_sign():
    from alac.net_amd.reverb import reverb_host, reverb_host_f32

    x = noise((3, 2, 777), 1)
    for a in (1.0, -1.0, 0.37, -3.5e-3, 1e4):
        h = np.full((3, 1, 1), a, dtype=np.float32)
        y = reverb_host(x, h)
        assert y.dtype == np.float64 and np.array_equal(y, np.sign(a) * x.astype(np.float64)), a
    # ... and behind other frames that are not valid
    h = np.array([[[-0.5, 9.0, 9.0]]] * 3, dtype=np.float32)
    assert np.array_equal(reverb_host(x, h, rir_lengths=[1, 1, 1]), -x.astype(np.float64))
    assert np.abs(reverb_host_f32(x, h, rir_lengths=[1, 1, 1]) + x).max() <= 4e-6


def test_the_direct_path_is_aligned_and_the_energy_is_one():
    from alac.net_amd.reverb import reverb_host

    T, K, d0 = 900, 300, 57
    x = np.zeros((1, 2, T), dtype=np.float32)
    x[0, 0, 400], x[0, 1, 123] = 1.0, -2.0
    rng = np.random.default_rng(3)
    h = (0.05 * rng.standard_normal((1, 1, K))).astype(np.float32)
    h[0, 0, d0] = 0.8
    y = reverb_host(x, h)
    assert int(np.argmax(np.abs(y[0, 0]))) == 400 and int(np.argmax(np.abs(y[0, 1]))) == 123
    g = 1.0 / np.sqrt(np.sum(h.astype(np.float64) ** 2))
    tap = float(h[0, 0, d0])
    assert abs(y[0, 0, 400] - g * tap) < 1e-15 and abs(y[0, 1, 123] + 2 * g * tap) < 1e-15
    # the response itself comes back from an impulse at 0, from its direct path on, with unit energy over what is kept
    x = np.zeros((1, 1, T), dtype=np.float32)
    x[0, 0, 0] = 1.0
    y = reverb_host(x, h)
    assert np.allclose(y[0, 0, :K - d0], g * h[0, 0, d0:].astype(np.float64), rtol=0, atol=1e-15) and not y[0, 0, K - d0:].any()
    # equal taps: the first; two channels: channel 0 decides, one gain for both
    h2 = np.zeros((1, 2, 8), dtype=np.float32)
    h2[0, 0, 2], h2[0, 0, 5], h2[0, 1, 4] = -1.0, 1.0, 3.0
    x = np.zeros((1, 2, 50), dtype=np.float32)
    x[0, :, 10] = 1.0
    y = reverb_host(x, h2)
    root = np.sqrt((1 + 1 + 9) / 2)
    assert y[0, 0, 10] == -1 / root and y[0, 0, 13] == 1 / root and y[0, 1, 12] == 3 / root and np.count_nonzero(y) == 3


def shifted_fftconvolve(x, h, v, vh):
    """One row by scipy: x [C, T], h [Ch, K] float32; float64 [C, T]"""
    from scipy.signal import fftconvolve

    C = x.shape[0]
    y = x.astype(np.float64)
    hh = h[:, :vh].astype(np.float64)
    d = int(np.argmax(np.abs(hh[0])))
    g = 1.0 / np.sqrt(np.sum(hh ** 2) / h.shape[0])
    for c in range(C):
        y[c, :v] = g * fftconvolve(x[c, :v].astype(np.float64), hh[c % h.shape[0]])[d:d + v]
    return y


def test_the_direct_sum_agrees_with_scipy():
    from alac.net_amd.reverb import reverb_host

    for C, Ch, T, K, seed in ((1, 1, 3000, 1200, 1), (2, 1, 2500, 700, 2), (2, 2, 1800, 2200, 3)):
        x = noise((2, C, T), seed)
        h = (np.random.default_rng(seed).standard_normal((2, Ch, K)) * np.exp(-np.arange(K) / (K / 5))).astype(np.float32)
        valid, hvalid = [T, T - 321], [K, K - 123]
        y = reverb_host(x, h, valid, hvalid)
        for b in range(2):
            want = shifted_fftconvolve(x[b], h[b], valid[b], hvalid[b])
            assert np.abs(y[b] - want).max() <= 1e-12 * np.abs(want).max(), (C, Ch, b)


def grid():
    """Every shape of the grid of tests/test_reverb.py, with its inputs"""
    from test_reverb import FRAMES, RIR_FRAMES, case

    for T in FRAMES:
        for K in RIR_FRAMES:
            turn = FRAMES.index(T) + 5 * RIR_FRAMES.index(K)
            for n, (C, Ch) in enumerate(((1, 1), (2, 1), (2, 2))):
                rows = 1 if (turn + n) % 3 == 0 else 3
                yield (T, K, C, Ch), case(T, K, C, Ch, rows, turn + n)


def test_the_twin_lies_inside_the_bound_on_the_whole_grid():
    from alac.net_amd.reverb import kappa, reverb_host, reverb_host_f32
    from test_reverb import stays

    worst = 0.0
    for tag, (x, h, valid, hvalid) in grid():
        y, dY = reverb_host(x, h, valid, hvalid, bound=True)
        t = reverb_host_f32(x, h, valid, hvalid)
        keep = stays(x, h, valid, hvalid)
        assert t.dtype == np.float32 and same_bits(t[keep], x[keep]) and not dY[keep].any() and (dY[~keep] > 0).all(), tag
        err = np.abs(t.astype(np.float64) - y)
        assert (err <= dY).all(), (tag, float((err / np.where(dY > 0, dY, 1)).max()))
        if (~keep).any():
            worst = max(worst, float((err[~keep] / dY[~keep]).max()))
    print(f"largest r_twin of the grid {worst:.3e}; c(N, 1) = {np.sqrt(N) * kappa(1) * 2 ** 24:.0f}, c(N, 8) = {np.sqrt(N) * kappa(8) * 2 ** 24:.0f}")
    assert 14000 < np.sqrt(N) * kappa(1) * 2 ** 24 < 17000                  # c(N, P) as the docstring states it


def test_the_rows_that_stay_stay_bit_for_bit():
    from alac.net_amd.reverb import reverb_host, reverb_host_f32

    T, K = 500, 200
    x = noise((6, 2, T), 9)
    x[:, :, 7] = -0.0
    h = (0.2 * noise((6, 1, K), 10)).astype(np.float32)
    h[4] = 0.0                                                             # silent
    h[5, 0, 3] = 3e38                                                      # e overflows in float32
    valid, hvalid = [T, 0, -4, T, T, T], [K, K, K, 0, K, K]
    for fn in (reverb_host, reverb_host_f32):
        y = fn(x, h, valid, hvalid)
        for b in (1, 2, 3, 4, 5):
            assert same_bits(y[b], x[b].astype(y.dtype)) and np.array_equal(np.signbit(y[b]), np.signbit(x[b])), (fn.__name__, b)
        assert not np.array_equal(y[0], x[0])
    y, dY = reverb_host(x, h, [300] * 6, None, bound=True)
    assert np.array_equal(y[:, :, 300:], x[:, :, 300:].astype(np.float64)) and not dY[:, :, 300:].any() and not dY[4].any()


def test_what_is_not_finite_stays_in_its_row():
    from alac.net_amd.reverb import reverb_host, reverb_host_f32

    T, K = 3 * H, 500
    x = noise((3, 1, T), 11)
    h = (0.2 * noise((3, 1, K), 12)).astype(np.float32)
    valid, hvalid = [T - 100, T, T], [K, K - 50, K]
    ref = reverb_host_f32(x, h, valid, hvalid)
    for bad in (NAN, INF):
        z, m = x.copy(), h.copy()
        z[0, 0, 1000] = bad
        m[1, 0, 17] = bad
        z[0, 0, T - 100:] = bad                                            # at and behind v, vh: never read
        m[1, 0, K - 50:] = bad
        for fn in (reverb_host, reverb_host_f32):
            y = fn(z, m, valid, hvalid)
            assert not np.isfinite(y[0, 0, :T - 100]).all(), (fn.__name__, bad)
            assert same_bits(y[1], x[1].astype(y.dtype)), "a response that is not finite leaves its row alone"
            assert np.isfinite(y[2]).all()
        assert same_bits(y[2], ref[2]) and not np.isfinite(reverb_host(z, m, valid, hvalid)[0, 0, 1000])


def test_the_host_functions_refuse_what_is_not_a_batch():
    from alac.net_amd.reverb import reverb_host, reverb_host_f32

    x, h = noise((2, 2, 40), 1), noise((2, 1, 10), 2)
    for fn in (reverb_host, reverb_host_f32):
        for args in ((x.astype(np.float64), h), (x, h.astype(np.float64)), (x[0], h[0]), (x, h[:1]), (x, noise((2, 3, 10), 3)), (x, h[..., :0]),
                     (x[..., :0], h), (x, h, [1]), (x, h, [1.0, 2.0]), (x, h, None, [1, 2, 3])):
            with pytest.raises(ValueError):
                fn(*args)


@pytest.mark.gpu
def test_draw_gives_the_same_draws_from_the_same_seed_whatever_p_is(tmp_path):
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(5)
    paths = []
    for k in range(5):
        pcm = torch.from_numpy((0.1 * rng.standard_normal((1, 400 + 50 * k))).astype(np.float32)).cuda()
        paths.append(str(tmp_path / f"rir{k}.m4a"))
        pkg.save(paths[-1], pcm, 16000)
    with pkg.Corpus(paths, device=0) as rirs:
        B = 64
        draws = {}
        for p in (0.0, 0.3, 1.0):
            aug = pkg.Reverb(rirs, p=p)
            for dev in ("cuda", "cpu"):
                g = torch.Generator(device=dev)
                g.manual_seed(1234)
                files, keep = aug.draw(B, generator=g)
                assert files.dtype == torch.int64 and keep.dtype == torch.bool and files.shape == keep.shape == (B,)
                assert files.device.type == "cuda" and keep.device.type == "cuda" and int(files.min()) >= 0 and int(files.max()) < 5
                u = torch.rand(B, generator=g, device=dev, dtype=torch.float64)     # the generator stands behind two draws of B
                draws[p, dev] = (files.cpu(), keep.cpu(), u.cpu())
        for dev in ("cuda", "cpu"):
            assert torch.equal(draws[0.0, dev][0], draws[0.3, dev][0]) and torch.equal(draws[0.3, dev][0], draws[1.0, dev][0])
            assert torch.equal(draws[0.0, dev][2], draws[0.3, dev][2]) and torch.equal(draws[0.3, dev][2], draws[1.0, dev][2])
            assert not draws[0.0, dev][1].any() and draws[1.0, dev][1].all() and 0 < int(draws[0.3, dev][1].sum()) < B
            assert bool((draws[0.3, dev][1] <= draws[1.0, dev][1]).all())
        with pytest.raises(ValueError):
            pkg.Reverb(rirs).draw(-1)
