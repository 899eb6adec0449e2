"""features.py without a device: the mel scales and the filterbank against known answers written out from their formulas, the
specification (logmel_host) against numpy's own padding and FFT, the derived bound against a plain float32 evaluation
(logmel_host_f32), and that evaluation as a yardstick: which broken tables it sees that the bound does not."""
import math

import numpy as np
import pytest

from alac.net_amd.features import (LogMel, dft_basis, frame_index, hann_window, hz_to_mel, logmel_host, logmel_host_f32,
                                   mel_filterbank, mel_to_hz)

SHAPES = [(400, 160, 80, 5000), (25, 10, 8, 333), (512, 128, 64, 4000), (2048, 512, 128, 9000), (16, 1, 4, 40)]

# (n_fft, hop, n_mels, L) by the branch of alac_features.hip each is there for; test_the_grid_is_what_it_claims holds every
# claim against the constants of alac_features.h.  tests/test_features_paths.py runs the kernel on them.
GRID = [
    (16, 2, 1, 50),             # hop 2, one mel
    (18, 3, 5, 60),             # even n_fft, one whole k-step left over
    (20, 20, 7, 130),           # hop = n_fft, fewer than 8 mels, a filter row of zeros
    (17, 5, 3, 70),             # odd n_fft whose only leftover step is the half one
    (33, 16, 9, 200),           # the same with two groups of eight k-steps
    (62, 31, 12, 700),          # 32 bins: one block, no clamped column
    (126, 64, 33, 1500),        # 64 bins: two blocks, no clamped column
    (63, 7, 12, 300),           # odd n_fft with 32 bins
    (402, 161, 80, 3000),       # one leftover step at the working size, a large odd hop
    (401, 160, 80, 3000),       # odd n_fft at the working size
    (510, 255, 40, 4000),       # exactly 8 blocks: one full round
    (1000, 250, 100, 5000),     # 4 leftover k-steps, 16 blocks: two full rounds
    (1022, 2, 8, 600),          # hop 2 under a long window, 301 frames in 10 tiles
    (1024, 1024, 17, 6000),     # 17 blocks: the last round has a single block
    (2046, 1024, 255, 9000),    # 1024 bins, 7 leftover k-steps, 255 mels
    (2048, 560, 256, 20000),    # the largest LDS layout of a full tile
    (2048, 561, 256, 20000),    # the last hop with a full tile
    (2048, 562, 256, 20000),    # the first hop with a shortened tile
    (2048, 580, 256, 20000),    # the largest LDS layout of all: a shortened tile, 8 samples short of the span limit
    (400, 160, 256, 3000),      # 45 filter rows of zeros
]


def test_mel_scales_known_answers():
    # slaney: 200 / 3 Hz per mel below 1000 Hz, then steps of ln(6.4) / 27 in ln f
    assert hz_to_mel(1000.0) == 15.0
    assert hz_to_mel(200.0 / 3.0) == pytest.approx(1.0, abs=1e-15) and hz_to_mel(500.0) == pytest.approx(7.5, abs=1e-14)
    assert hz_to_mel(0.0) == 0.0
    assert hz_to_mel(6400.0) == pytest.approx(15.0 + 27.0, rel=1e-14)                 # ln(6.4) / step = 27
    assert hz_to_mel(1000.0 * math.exp(math.log(6.4) / 27.0)) == pytest.approx(16.0, rel=1e-14)
    assert mel_to_hz(15.0) == 1000.0 and mel_to_hz(42.0) == pytest.approx(6400.0, rel=1e-13)
    assert mel_to_hz(3.0) == pytest.approx(200.0, rel=1e-15)
    # htk: 2595 log10(1 + f / 700)
    assert hz_to_mel(700.0, "htk") == pytest.approx(2595.0 * math.log10(2.0), rel=1e-15)
    assert hz_to_mel(0.0, "htk") == 0.0 and hz_to_mel(6300.0, "htk") == pytest.approx(2595.0, rel=1e-15)
    for scale in ("slaney", "htk"):
        f = np.array([0.0, 10.0, 999.0, 1000.0, 1001.0, 4000.0, 8000.0, 24000.0])
        assert np.allclose(mel_to_hz(hz_to_mel(f, scale), scale), f, rtol=1e-12, atol=1e-9)
    with pytest.raises(ValueError):
        hz_to_mel(1.0, "bark")


@pytest.mark.parametrize("scale", ["slaney", "htk"])
def test_filters_are_triangles_between_their_three_points(scale):
    sr, n_fft, n_mels = 16000, 400, 40
    fb = mel_filterbank(sr, n_fft, n_mels, f_min=20.0, f_max=7600.0, scale=scale, norm=None)
    assert fb.shape == (n_mels, n_fft // 2 + 1) and fb.dtype == np.float32
    pts = mel_to_hz(np.linspace(hz_to_mel(20.0, scale), hz_to_mel(7600.0, scale), n_mels + 2), scale)
    f = np.arange(n_fft // 2 + 1) * sr / n_fft
    for m in range(n_mels):
        lo, mid, hi = pts[m:m + 3]
        want = np.where(f <= mid, (f - lo) / (mid - lo), (hi - f) / (hi - mid)).clip(min=0.0)
        assert np.allclose(fb[m], want, rtol=0, atol=1e-7), m
        assert (fb[m][(f <= lo) | (f >= hi)] == 0).all() and (fb[m] >= 0).all() and fb[m].max() <= 1.0
        up = fb[m][(f >= lo) & (f <= mid)]
        down = fb[m][(f >= mid) & (f <= hi)]
        assert (np.diff(up) >= 0).all() and (np.diff(down) <= 0).all()


def test_peak_on_a_bin_centre_has_weight_one():
    # htk mel points chosen so that a filter's middle point is a bin: sr 16000, n_fft 16: bins every 1000 Hz; one filter from
    # 1000 over f_1 to f_max, and f_1 is a bin when mel(f_1) is the mean of mel(1000) and mel(f_max): f_max = 700 (3.9^2 / 2.43 - 1)
    # puts it at 2000 Hz, since (1 + 2000 / 700)^2 = (1 + 1000 / 700) (1 + f_max / 700)
    f_max = 700.0 * ((1 + 2000.0 / 700.0) ** 2 / (1 + 1000.0 / 700.0) - 1)
    fb = mel_filterbank(16000, 16, 1, f_min=1000.0, f_max=f_max, scale="htk", norm=None)
    assert fb[0, 2] == pytest.approx(1.0, abs=1e-6) and fb[0, 1] == 0.0 and 0 < fb[0, 3] < 1
    # slaney below 1000 Hz is linear: 0 .. 500 .. 1000 over bins every 250 Hz
    fb = mel_filterbank(8000, 32, 1, f_min=0.0, f_max=1000.0, norm=None)
    assert np.allclose(fb[0, :6], [0.0, 0.5, 1.0, 0.5, 0.0, 0.0], atol=1e-7)


def test_slaney_norm_is_two_over_the_width():
    sr, n_fft, n_mels = 16000, 2048, 20
    plain = mel_filterbank(sr, n_fft, n_mels, norm=None).astype(np.float64)
    normed = mel_filterbank(sr, n_fft, n_mels, norm="slaney").astype(np.float64)
    pts = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(8000.0), n_mels + 2))
    assert np.allclose(normed, plain * (2.0 / (pts[2:] - pts[:-2]))[:, None], rtol=1e-6, atol=0)
    # ... which gives every filter unit area in Hz: the bins are a Riemann sum of it (7.8 Hz apart, filters 200 Hz and wider)
    area = normed.sum(axis=1) * sr / n_fft
    assert np.allclose(area, 1.0, atol=2e-3), area
    with pytest.raises(ValueError):
        mel_filterbank(sr, n_fft, n_mels, norm="l2")


def test_tables():
    sp = LogMel(16000)
    assert (sp.n_fft, sp.hop_length, sp.n_mels, sp.n_bins, sp.log, sp.floor) == (400, 160, 80, 201, "ln", 1e-10)
    assert sp.window.shape == (400,) and sp.basis.shape == (400, 402) and sp.fb.shape == (80, 201)
    assert all(a.dtype == np.float32 and not a.flags.writeable for a in (sp.window, sp.basis, sp.fb))
    n = np.arange(400)
    assert np.array_equal(sp.window, (0.5 - 0.5 * np.cos(2 * np.pi * n / 400)).astype(np.float32))
    assert sp.window[0] == 0 and sp.window[200] == 1 and sp.window[1] == sp.window[399]
    # the angle is reduced in integers: n k = 399 * 200 is the angle of 200, half a turn, and the cosine is -1 exactly
    b = sp.basis
    assert b[100, 201 + 1] == -1 and b[200, 1] == -1 and b[399, 200] == -1 and abs(b[100, 1]) < 1e-16 and abs(b[399, 201 + 200]) < 1e-15
    assert (b[:, 0] == 1).all() and (b[:, 201] == 0).all()
    nk = (np.arange(400)[:, None] * np.arange(201)[None, :]) % 400
    assert np.array_equal(b[:, :201], np.cos(2 * np.pi * (nk / 400)).astype(np.float32))
    assert np.array_equal(b[:, 201:], (-np.sin(2 * np.pi * (nk / 400))).astype(np.float32))
    assert np.array_equal(b, dft_basis(400)) and np.array_equal(sp.window, hann_window(400))
    assert np.array_equal(sp.fb, mel_filterbank(16000, 400, 80))
    with pytest.raises(AttributeError):
        sp.n_fft = 512
    with pytest.raises(ValueError):
        sp.window[0] = 1.0
    assert sp.frames(32000) == 201 and sp.frames(159) == 1 and sp.frames(160) == 2
    assert LogMel(16000, log=None).log_mode == 0 and sp.log_mode == 1 and LogMel(16000, log="log10").log_mode == 2
    own = np.ones((3, 201), dtype=np.float64)
    assert LogMel(16000, filterbank=own).n_mels == 3 and LogMel(16000, filterbank=own).fb.dtype == np.float32


@pytest.mark.parametrize("kw", [
    dict(n_fft=15), dict(n_fft=2049), dict(n_fft=400.0), dict(hop_length=0), dict(hop_length=401), dict(n_mels=0), dict(n_mels=257),
    dict(floor=0.0), dict(floor=-1e-10), dict(floor=float("inf")), dict(floor=float("nan")), dict(f_min=-1.0),
    dict(f_min=4000.0, f_max=4000.0), dict(f_min=5000.0, f_max=4000.0), dict(f_max=8000.5), dict(log="log2"), dict(scale="bark"),
    dict(norm="l1"), dict(sample_rate=0), dict(filterbank=np.ones((3, 200))), dict(filterbank=np.ones((257, 201))),
    dict(filterbank=np.ones(201))])
def test_limits_raise_value_error(kw):
    with pytest.raises(ValueError):
        LogMel(**{"sample_rate": 16000, **kw})
    fb_kw = {k: v for k, v in kw.items() if k in ("n_fft", "n_mels", "f_min", "f_max", "scale", "norm")}
    if fb_kw:
        with pytest.raises(ValueError):
            mel_filterbank(16000, fb_kw.pop("n_fft", 400), fb_kw.pop("n_mels", 80), **fb_kw)


def test_limits_are_inclusive():
    for kw in (dict(n_fft=16, hop_length=16, n_mels=1), dict(n_fft=2048, hop_length=2048, n_mels=256), dict(hop_length=1),
               dict(f_min=0.0, f_max=8000.0)):
        LogMel(16000, **kw)


@pytest.mark.parametrize("n_fft,hop,n_mels,L", SHAPES + [(400, 160, 80, 201), (25, 10, 8, 13), (16, 16, 4, 9)])
def test_power_matches_numpys_padding_and_fft(n_fft, hop, n_mels, L):
    """The framing is np.pad(reflect) by n_fft // 2 and the DFT is rfft: with a filterbank that picks single bins the
    specification's mel power is the periodogram itself, within 1e-7 of its peak.  (L = n_fft // 2 + 1: the shortest row, where
    a frame reflects at both ends.)"""
    rng = np.random.default_rng(L)
    x = rng.uniform(-1, 1, L).astype(np.float32)
    n_bins = n_fft // 2 + 1
    sp = LogMel(16000, n_fft, hop, filterbank=np.eye(n_bins, dtype=np.float32)[:min(n_bins, 256)], log=None)
    T = sp.frames(L)
    assert T == 1 + L // hop
    got = logmel_host(x, sp)
    assert got.shape == (sp.n_mels, T)
    # even n_fft: torch.stft's frame count; an odd one has L // hop + 1 frames here too, which needs one more sample of padding
    padded = np.pad(x.astype(np.float64), (n_fft // 2, n_fft // 2 + n_fft % 2), mode="reflect")
    w = hann_window(n_fft).astype(np.float64)
    frames = np.stack([padded[t * hop:t * hop + n_fft] for t in range(T)])
    want = np.abs(np.fft.rfft(frames * w, axis=1)) ** 2          # [T, n_bins]
    err = np.abs(got - want.T[:sp.n_mels])
    print(f"({n_fft},{hop}) L {L}: max err {err.max():.3e}, peak {want.max():.3e}")
    assert err.max() <= 1e-7 * want.max()


def test_a_tap_one_reflection_does_not_reach_is_zero():
    idx, inside = frame_index(13, 25, 13)               # the second frame is centred on L = 13: its last tap is index L - 1 + 13
    assert idx.shape == (2, 25) and inside.sum() == 49 and not inside[1, 24]
    assert idx[0].tolist() == list(range(12, 0, -1)) + list(range(13))
    assert idx[1, :24].tolist() == list(range(1, 13)) + list(range(11, -1, -1))
    idx, inside = frame_index(333, 25, 10)
    assert inside.all() and idx.shape == (34, 25)


def test_log_and_floor():
    x = np.random.default_rng(1).uniform(-1, 1, (2, 3000)).astype(np.float32)
    M = logmel_host(x, LogMel(16000, log=None))
    assert M.shape == (2, 80, 19) and M.dtype == np.float64
    assert np.allclose(logmel_host(x, LogMel(16000)), np.log(M), rtol=1e-14)
    assert np.allclose(logmel_host(x, LogMel(16000, log="log10", floor=1.0)), np.log10(np.maximum(M, 1.0)), rtol=1e-14)
    silent = np.zeros(3000, dtype=np.float32)
    assert (logmel_host(silent, LogMel(16000)) == np.log(float(np.float32(1e-10)))).all()
    assert (logmel_host(silent, LogMel(16000, log=None)) == 0).all()
    with pytest.raises(ValueError):
        logmel_host(x[:, :200], LogMel(16000))
    with pytest.raises(ValueError):
        logmel_host(x.astype(np.float64), LogMel(16000))


float32_serial = logmel_host_f32           # the specification in plain float32, one operation at a time (features.py)


@pytest.mark.parametrize("n_fft,hop,n_mels,L", SHAPES + GRID)
def test_a_float32_evaluation_stays_inside_the_bound(n_fft, hop, n_mels, L):
    """(On the grid a filter may be all zeros -- no bin between its points: there M = dM = 0 and the evaluation gives 0; the
    bound is asserted positive and below 0.1 M on all other elements, which on SHAPES are all.  The grid's noise is the first
    row of what tests/test_features_paths.py gives the kernel.)"""
    sp = LogMel(16000, n_fft, hop, n_mels, log=None)
    rng = np.random.default_rng(n_fft + ((n_fft, hop, n_mels, L) in SHAPES))
    tone = np.sin(2 * np.pi * (n_fft // 8) * np.arange(L) / n_fft).astype(np.float32)
    empty = (sp.fb == 0).all(axis=1)
    assert not empty.any() or (n_fft, hop, n_mels, L) in GRID
    for name, x in (("noise", rng.uniform(-1, 1, L).astype(np.float32)), ("tone", tone)):
        M, dM = logmel_host(x, sp, bound=True)
        got = float32_serial(x, sp)
        err = np.abs(got.astype(np.float64) - M)
        ratio = np.max(err / np.maximum(dM, 1e-300))
        print(f"({n_fft},{hop},{n_mels}) {name}: max err / dM {ratio:.3f}")
        assert (err <= dM).all()
        assert (M[empty] == 0).all() and (dM[empty] == 0).all() and (got[empty] == 0).all()
        assert (dM[~empty] > 0).all() and (dM[~empty] <= 0.1 * M[~empty]).all() if name == "noise" else True
    # the centre tap dropped is outside the bound in most elements: it does not hide a bug
    x = rng.uniform(-1, 1, L).astype(np.float32)
    M, dM = logmel_host(x, sp, bound=True)
    broken = LogMel(16000, n_fft, hop, n_mels, log=None)
    w = np.array(broken.window)
    w[n_fft // 2] = 0.0
    object.__setattr__(broken, "window", w)
    assert (np.abs(logmel_host(x, broken) - M) > dM)[~empty].mean() > 0.5


def test_crops_take_features_and_keep_their_other_arguments():
    import inspect

    import alac.net_amd as pkg

    for fn, head in ((pkg.Corpus.crops, ["self", "files", "frame_offsets", "num_frames", "dtype", "out", "check"]),
                     (pkg.Corpus.random_crops, ["self", "batch", "num_frames", "generator", "dtype", "out", "check"])):
        p = inspect.signature(fn).parameters
        assert list(p)[:7] == head and p["features"].default is None
        assert p["sample_rate"].default is None and p["mono"].default is False
    assert pkg.log_mel and pkg.LogMel is LogMel and pkg.mel_filterbank is mel_filterbank and pkg.logmel_host is logmel_host


def _broken(sp, window=None, fb=None):
    """sp with one of its tables replaced (a specification with a bug in it)"""
    b = LogMel(16000, sp.n_fft, sp.hop_length, sp.n_mels, log=None)
    for name, table in (("window", window), ("fb", fb)):
        if table is not None:
            object.__setattr__(b, name, table)
    return b


def _mutations(sp):
    """name -> a broken specification, tables changed only: (a) the last tap dropped; (b) the first bin of the second block of
    32 removed from every filter, as a round of the mel chain that starts one bin late would (None where there is one block);
    (c) the tap nearest either end whose window weight is at least 1e-3 dropped, and its mirror image at the front"""
    w = np.array(sp.window)
    last = sp.n_fft - 1 - int(np.argmax(w[::-1] >= 1e-3))
    first = int(np.argmax(w >= 1e-3))
    assert w[last] >= 1e-3 and (w[last + 1:] < 1e-3).all() and sp.n_fft - 1 - last <= first
    out = {}
    for name, taps in (("a", [sp.n_fft - 1]), ("c", [last]), ("c front", [first])):
        v = w.copy()
        v[taps] = 0.0
        out[name] = _broken(sp, window=v)
    out["b"] = None
    if sp.n_bins > 32:
        fb = np.array(sp.fb)
        assert (fb[:, 32] > 0).any()
        fb[:, 32] = 0.0
        out["b"] = _broken(sp, fb=fb)
    return out


# What the bound dM alone (tests/test_features.py before the twin) makes of each mutation: True = it is blind to it, the broken
# evaluation is inside dM in every element.  Measured here, with the reasons:
#   (400, 160, 80): dM / M is 0.5 to 1.6 %, a tap of weight 6e-5 (a) or 1.5e-3 (c) moves the power by less.  A whole bin gone from
#   the two filters that hold it (b) is far outside.
#   (126, 64, 33) and (25, 10, 8): dM / M is below 1e-3 with so short a chain of roundings, and the last tap weighs 6e-4 and
#   1.6e-2: the bound sees a lost tap already.  (25, 10, 8) has 13 bins, one block: (b) does not exist there, so (126, 64, 33),
#   the smallest grid shape with a second block, stands in for it.
BLIND = {(400, 160, 80, 5000): {"a": True, "b": False, "c": True, "c front": True},
         (126, 64, 33, 1500): {"a": False, "b": False, "c": False, "c front": False},
         (25, 10, 8, 333): {"a": False, "b": None, "c": False, "c front": False}}


@pytest.mark.parametrize("shape", list(BLIND))
def test_the_twin_sees_what_the_bound_does_not(shape):
    """A float32 evaluation of a specification with one table entry wrong, against the true M: every mutation is outside
    4 r_ref, r_ref the twin's own max err / dM on the same input, so the test of r_gpu <= 4 r_ref fails a kernel that has it.
    At the working size the lost taps are inside dM in every element -- the bound alone passes them.  BLIND says where the
    bound is blind and where it is not, and why."""
    n_fft, hop, n_mels, L = shape
    sp = LogMel(16000, n_fft, hop, n_mels, log=None)
    x = np.random.default_rng(n_fft + 1).uniform(-1, 1, L).astype(np.float32)
    M, dM = logmel_host(x, sp, bound=True)
    r_ref = float(np.max(np.abs(logmel_host_f32(x, sp) - M) / dM))
    assert 0 < r_ref < 0.25                                     # 4 r_ref is inside the bound: the yardstick is the tighter one
    seen_only_by_the_twin = 0
    for name, broken in _mutations(sp).items():
        assert (broken is None) == (BLIND[shape][name] is None)
        if broken is None:
            continue
        err = np.abs(logmel_host_f32(x, broken) - M)
        ratio = float(np.max(err / dM))
        inside = bool((err <= dM).all())
        print(f"({n_fft},{hop},{n_mels}) {name}: inside dM {inside}, max err / dM {ratio:.4f} against 4 r_ref = {4 * r_ref:.4f}")
        assert inside == BLIND[shape][name], name
        assert ratio > 4 * r_ref, name
        seen_only_by_the_twin += inside
    assert seen_only_by_the_twin == sum(v is True for v in BLIND[shape].values())


def test_the_grid_is_what_it_claims():
    """Every branch GRID names, from the constants of alac_features.h and alac_features.hip: a later change of one of them
    cannot quietly turn two entries into duplicates."""
    from test_features import header_constant, kernel_blocks, kernel_lds_bytes, kernel_tile

    tile, block, per_round = (header_constant("ALAC_FEATURES_" + n) for n in ("TILE", "BLOCK", "ROUND_BLOCKS"))
    ahead = header_constant("AHEAD", "alac_features.hip")
    assert (tile, block, per_round, ahead) == (32, 32, 8, 8)
    assert len(set(GRID)) == len(GRID) and not set(GRID) & set(SHAPES)

    def facts(n_fft, hop, n_mels, L):
        T = 1 + L // hop
        return dict(left=(n_fft // 2) % ahead, half=n_fft % 2, blocks=kernel_blocks(n_fft), clamped=(n_fft // 2 + 1) % block != 0,
                    tile=kernel_tile(n_fft, hop), tiles=-(-T // kernel_tile(n_fft, hop)), frames=T,
                    empty=int((LogMel(16000, n_fft, hop, n_mels).fb == 0).all(axis=1).sum()))

    want = {
        (16, 2, 1, 50): dict(left=0, half=0, blocks=1),
        (18, 3, 5, 60): dict(left=1, half=0),
        (20, 20, 7, 130): dict(left=2, half=0, empty=1),
        (17, 5, 3, 70): dict(left=0, half=1),
        (33, 16, 9, 200): dict(left=0, half=1),
        (62, 31, 12, 700): dict(blocks=1, clamped=False),
        (126, 64, 33, 1500): dict(blocks=2, clamped=False),
        (63, 7, 12, 300): dict(blocks=1, clamped=False, half=1),
        (402, 161, 80, 3000): dict(left=1, half=0, blocks=7),
        (401, 160, 80, 3000): dict(left=0, half=1, blocks=7),
        (510, 255, 40, 4000): dict(blocks=per_round, clamped=False),
        (1000, 250, 100, 5000): dict(left=4, blocks=2 * per_round, clamped=True),
        (1022, 2, 8, 600): dict(blocks=2 * per_round, clamped=False, frames=301, tiles=10),
        (1024, 1024, 17, 6000): dict(blocks=2 * per_round + 1, tile=19),
        (2046, 1024, 255, 9000): dict(left=7, blocks=4 * per_round, clamped=False, tile=18),
        (2048, 560, 256, 20000): dict(tile=tile, tiles=2, blocks=4 * per_round + 1),
        (2048, 561, 256, 20000): dict(tile=tile, tiles=2),
        (2048, 562, 256, 20000): dict(tile=tile - 1, tiles=2),
        (2048, 580, 256, 20000): dict(tile=tile - 1, tiles=2),
        (400, 160, 256, 3000): dict(empty=45),
    }
    assert set(want) == set(GRID)
    for shape, claims in want.items():
        got = facts(*shape)
        assert {k: got[k] for k in claims} == claims, shape
    # every even n_fft of SHAPES has n_fft / 2 divisible by AHEAD, none of its n_bins is a multiple of the block: what the grid adds
    assert all(facts(*s)["left"] == 0 and facts(*s)["clamped"] for s in SHAPES if s[0] % 2 == 0)
    # the layouts: 561 is the last hop with a full tile at n_fft 2048; 560 has the largest layout of all full tiles (an even hop
    # is skewed), and the largest of all is a shortened tile; all fit a CU's LDS
    most, lds_max = header_constant("ALAC_FEATURES_MAX_SPAN"), header_constant("ALAC_FEATURES_LDS_MAX")
    assert (tile - 1) * 561 + 2048 <= most < (tile - 1) * 562 + 2048
    sizes = {(n_fft, hop): kernel_lds_bytes(n_fft, hop, 256) for n_fft in (2047, 2048) for hop in range(1, n_fft + 1)}
    full = {k: v for k, v in sizes.items() if kernel_tile(*k) == tile}
    assert max(full, key=full.get) == (2048, 560) and full[2048, 560] == 151500
    assert max(sizes, key=sizes.get) == (2048, 580) and sizes[2048, 580] == 151656 <= lds_max == 160 << 10


def test_what_is_not_finite_stays_in_its_frames_and_is_never_hidden():
    """The specification on a NaN and on an infinity (features.py): NaN in every element of the frames with a tap on it -- the
    tap of weight zero too -- with and without a log; every other frame is bit for bit the clean signal's."""
    n_fft, hop, L, i = 400, 160, 4000, 2050
    x = np.random.default_rng(2).uniform(-1, 1, L).astype(np.float32)
    t = np.arange(1 + L // hop)
    hit = (t * hop - n_fft // 2 <= i) & (i < t * hop - n_fft // 2 + n_fft)
    assert t[hit].tolist() == [12, 13, 14]
    for log in (None, "ln", "log10"):
        sp = LogMel(16000, log=log)
        clean = logmel_host(x, sp)
        for bad in (np.nan, np.inf, -np.inf):
            y = x.copy()
            y[i] = bad
            with np.errstate(invalid="ignore"):
                got = logmel_host(y, sp)
            assert np.isnan(got[:, hit]).all() and np.array_equal(got[:, ~hit], clean[:, ~hit])
    # the tap of weight zero: frame 14 starts on sample 2040
    y = x.copy()
    y[14 * hop - n_fft // 2] = np.inf
    with np.errstate(invalid="ignore"):
        got = logmel_host(y, LogMel(16000))
    assert np.isnan(got[:, 12:15]).all() and np.isfinite(got[:, :12]).all() and np.isfinite(got[:, 15:]).all()
