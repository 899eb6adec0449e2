"""fbank.py without a device: Kaldi's framing and reflection, mel banks and windows, the GEMM formulation against a literal
zero-padded FFT of every frame, the float32 twin against the derived bound, and the refusals."""
import numpy as np
import pytest

from alac.net_amd.fbank import (FLOOR, KaldiFbank, fbank_frame_index, fbank_host, fbank_host_f32, fbank_lengths, kaldi_mel,
                                kaldi_mel_banks, kaldi_window)

# (win, hop, round_to_power_of_two, n_mels, L): the shapes tests/test_fbank.py runs on the device
GRID = [(400, 160, True, 80, 5000), (25, 10, True, 8, 333), (16, 1, True, 4, 40), (512, 128, True, 64, 4000),
        (400, 160, False, 80, 5000), (2048, 512, True, 40, 9000)]
# (win, hop, n_mels, n_ceps, frames with snip_edges): one shape per code path of alac_fbank.hip and alac_mfcc.hip that depends on
# the tile, the lane or the skew; tests/test_kaldi_paths.py runs them on the device, tests/test_mfcc_spec.py on the CPU as here
PATHS = [(63, 7, 12, 12, 2 * 32 + 7),        # an odd hop above 1: no skew, q and r are real; odd K, whole k-steps in the remainder
         (401, 161, 40, 13, 2 * 32 + 3),     # an odd window and an odd hop at speech size: 200 pairs and an odd tail, two rounds
         (64, 16, 8, 8, 2 * 32 + 7),         # an even hop that divides the window: r == 0 at every hop boundary, two words back
         (16, 16, 4, 4, 70),                 # hop == win: a sample belongs to one frame, q stays 0
         (2048, 600, 40, 20, 30 + 3),        # a tile of 30 frames with the taps at the cap, two tiles
         (2048, 2048, 23, 13, 9 + 2),        # a tile of 9, hop == win at the largest window
         (2048, 560, 256, 23, 33)]           # the largest LDS layout: 256 filters, the span at the cap, the kernel's own floats


def paths_length(win, hop, frames):
    """The L that gives `frames` frames with snip_edges, and three samples to spare"""
    return win + (frames - 1) * hop + 3


PATH_GRID = [(win, hop, True, n_mels, paths_length(win, hop, frames)) for win, hop, n_mels, _, frames in PATHS]


def noise(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.mark.parametrize("win,hop", [(400, 160), (25, 10), (16, 1), (32, 32)])
def test_frame_counts_and_first_samples(win, hop):
    for L in (1, win - 1, win, win + hop - 1, win + hop):
        snip = KaldiFbank(16000, win, hop, 4, snip_edges=True)
        T = 0 if L < win else 1 + (L - win) // hop
        assert snip.frames(L) == T and isinstance(snip.frames(L), int)
        idx = fbank_frame_index(L, snip)
        assert idx.shape == (T, win)
        if T:
            assert idx[:, 0].tolist() == [t * hop for t in range(T)] and idx.max() == (T - 1) * hop + win - 1 < L
            assert (np.diff(idx, axis=1) == 1).all()
        centred = KaldiFbank(16000, win, hop, 4, snip_edges=False)
        T = (L + hop // 2) // hop
        assert centred.frames(L) == T
        idx = fbank_frame_index(L, centred)
        assert idx.shape == (T, win) and (T == 0 or (idx.min() >= 0 and idx.max() < L))
        first = hop // 2 - win // 2
        for t in range(T):                                     # frame t starts at t hop + hop // 2 - win // 2, reflected by -g - 1
            g = t * hop + first
            if -L <= g < L:
                assert idx[t, 0] == (g if g >= 0 else -g - 1)
    assert snip.min_frames == win and snip.frames(snip.min_frames) == 1 and snip.frames(snip.min_frames - 1) == 0
    assert centred.frames(centred.min_frames) == 1 and centred.frames(centred.min_frames - 1) == 0
    lens = np.array([-1, 0, 1, win - 1, win, win + hop, 10 * win])
    for spec in (snip, centred):
        want = [-1] + [spec.frames(int(n)) for n in lens[1:]]
        assert fbank_lengths(lens, spec).tolist() == want and fbank_lengths(lens, spec).dtype == np.int64
        assert spec.frames(lens[1:]).tolist() == want[1:]
        import torch
        got = fbank_lengths(torch.from_numpy(lens), spec)
        assert got.dtype == torch.int64 and got.tolist() == want
    with pytest.raises(ValueError):
        fbank_lengths(np.array([1.0]), snip)


def test_closed_form_reflection_is_kaldis_loop():
    """L = 5 under a window of 25: every index is reflected several times"""
    L, win, hop = 5, 25, 10
    spec = KaldiFbank(16000, win, hop, 4, snip_edges=False)
    idx = fbank_frame_index(L, spec)
    assert idx.shape == ((L + hop // 2) // hop, win) == (1, 25)
    for t in range(idx.shape[0]):
        for n in range(win):
            g = t * hop + hop // 2 - win // 2 + n
            while g < 0 or g >= L:                              # kaldi/src/feat/feature-window.cc, ExtractWindow
                g = -g - 1 if g < 0 else 2 * L - 1 - g
            assert idx[t, n] == g, (t, n)
    assert idx.min() == 0 and idx.max() == L - 1
    for L, win, hop in ((7, 16, 3), (1, 16, 1), (40, 16, 16)):
        spec = KaldiFbank(8000, win, hop, 4, snip_edges=False)
        idx = fbank_frame_index(L, spec)
        for t in range(idx.shape[0]):
            for n in range(win):
                g = t * hop + hop // 2 - win // 2 + n
                while g < 0 or g >= L:
                    g = -g - 1 if g < 0 else 2 * L - 1 - g
                assert idx[t, n] == g


def test_mel_banks():
    for rate, n_fft, n_mels in ((16000, 512, 80), (16000, 512, 23), (8000, 256, 40), (16000, 400, 80), (16000, 2048, 40)):
        fb = kaldi_mel_banks(rate, n_fft, n_mels)
        assert fb.shape == (n_mels, n_fft // 2 + 1) and fb.dtype == np.float32
        assert (fb >= 0).all() and (fb <= 1).all()
        assert (fb[:, -1] == 0).all()                           # the Nyquist bin
        assert (fb.sum(axis=1) > 0).all(), (rate, n_fft, n_mels)  # no filter is empty
        # between the first and the last centre a bin's weights over the (two) filters that cover it sum to 1
        lo, hi = kaldi_mel(20.0), kaldi_mel(rate / 2)
        delta = (hi - lo) / (n_mels + 1)
        z = kaldi_mel(np.arange(n_fft // 2) * rate / n_fft)
        inside = (z >= lo + delta) & (z <= lo + n_mels * delta)
        assert inside.sum() > n_mels // 2
        assert np.abs(fb[:, :n_fft // 2].astype(np.float64).sum(axis=0)[inside] - 1.0).max() < 1e-6
        assert ((fb > 0).sum(axis=0) <= 2).all()
    # by hand: 4 filters over 0 .. 4000 Hz at 8000 Hz, 16 bins of 250 Hz
    fb = kaldi_mel_banks(8000, 32, 4, low_freq=0.0)
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    d = mel(4000.0) / 5
    for k in range(17):
        z = mel(250.0 * k)
        for m in range(4):
            left, centre, right = m * d, (m + 1) * d, (m + 2) * d
            w = 0.0
            if k < 16 and left < z <= centre:
                w = (z - left) / d
            elif k < 16 and centre < z < right:
                w = (right - z) / d
            assert abs(float(fb[m, k]) - w) < 1e-7, (m, k)
    assert fb[0, 0] == 0 and fb[0, 1] > 0 and np.argmax(fb[3]) > np.argmax(fb[0])
    # high_freq <= 0 is an offset from Nyquist
    assert np.array_equal(kaldi_mel_banks(16000, 512, 23, 20.0, -400.0), kaldi_mel_banks(16000, 512, 23, 20.0, 7600.0))
    for bad in (dict(low_freq=-1.0), dict(low_freq=8000.0), dict(high_freq=8001.0), dict(high_freq=-8000.0), dict(high_freq=10.0)):
        with pytest.raises(ValueError):
            kaldi_mel_banks(16000, 512, 23, **bad)


def test_windows_at_a_few_taps():
    N = 400
    han = kaldi_window("hanning", N).astype(np.float64)
    assert han[0] == 0 and abs(han[N - 1]) < 1e-7 and abs(han[100] - (0.5 - 0.5 * np.cos(2 * np.pi * 100 / 399))) < 1e-7
    assert np.abs(kaldi_window("povey", N) - han ** 0.85).max() < 1e-6
    ham = kaldi_window("hamming", N)
    assert abs(ham[0] - 0.08) < 1e-7 and abs(ham[7] - (0.54 - 0.46 * np.cos(2 * np.pi * 7 / 399))) < 1e-7
    bl = kaldi_window("blackman", N)
    assert abs(bl[0]) < 1e-7 and abs(bl[50] - (0.42 - 0.5 * np.cos(2 * np.pi * 50 / 399) + 0.08 * np.cos(4 * np.pi * 50 / 399))) < 1e-7
    assert (kaldi_window("rectangular", 25) == 1).all()
    for w in ("povey", "hanning", "hamming", "blackman"):       # symmetric, the peak in the middle
        v = kaldi_window(w, 25)
        assert v.dtype == np.float32 and np.allclose(v, v[::-1], atol=1e-7) and np.argmax(v) == 12
    with pytest.raises(ValueError):
        kaldi_window("hann", 25)


@pytest.mark.parametrize("win,hop,pow2,n_mels,L", GRID)
def test_the_gemm_is_the_zero_padded_transform(win, hop, pow2, n_mels, L):
    rng = np.random.default_rng(win + hop)
    x = noise(rng, L)
    for snip in (True, False):
        spec = KaldiFbank(16000, win, hop, n_mels, round_to_power_of_two=pow2, snip_edges=snip, log=False)
        assert spec.n_fft == (1 << (win - 1).bit_length() if pow2 else win) and spec.basis.shape == (win, 2 * spec.n_bins)
        M = fbank_host(x, spec)
        assert M.shape == (n_mels, spec.frames(L))
        want = np.empty_like(M)
        for t in range(M.shape[1]):                              # the literal formulation of one frame
            g0 = t * hop + (0 if snip else hop // 2 - win // 2)
            frame = np.empty(win)
            for n in range(win):
                g = g0 + n
                while g < 0 or g >= L:
                    g = -g - 1 if g < 0 else 2 * L - 1 - g
                frame[n] = 32768.0 * float(x[g])
            frame -= frame.sum() / win
            frame = frame - float(np.float32(0.97)) * np.concatenate([frame[:1], frame[:-1]])
            frame *= kaldi_window("povey", win).astype(np.float64)
            padded = np.zeros(spec.n_fft)
            padded[:win] = frame
            want[:, t] = spec.fb.astype(np.float64) @ (np.abs(np.fft.rfft(padded)) ** 2)
        rel = np.abs(M - want).max(axis=0) / want.max(axis=0)
        print(f"({win},{hop},{spec.n_fft},{n_mels}) snip {snip}: {rel.max():.2e}")
        assert rel.max() <= 1e-4
        logged = fbank_host(x, KaldiFbank(16000, win, hop, n_mels, round_to_power_of_two=pow2, snip_edges=snip))
        assert np.array_equal(logged, np.log(np.maximum(M, FLOOR)))
        mag = fbank_host(x, KaldiFbank(16000, win, hop, n_mels, round_to_power_of_two=pow2, snip_edges=snip, log=False, use_power=False))
        assert mag.shape == M.shape and (mag <= np.sqrt(M * spec.fb.astype(np.float64).sum(axis=1)[:, None]) * (1 + 1e-9) + 1e-9).all()


@pytest.mark.parametrize("win,hop,pow2,n_mels,L", GRID + PATH_GRID)
def test_the_float32_twin_is_inside_the_bound(win, hop, pow2, n_mels, L):
    """PATH_GRID as well: what tests/test_kaldi_paths.py rests on holds for the reference alone -- the twin inside dM (at
    2048 taps the device test leaves the twin to this one) and the narrow share that keeps its log check from being vacuous"""
    rng = np.random.default_rng(win + hop if (win, hop, pow2, n_mels, L) in PATH_GRID else win)
    x = noise(rng, 1, L)
    for snip in (True, False):
        spec = KaldiFbank(16000, win, hop, n_mels, round_to_power_of_two=pow2, snip_edges=snip, log=False)
        M, dM = fbank_host(x, spec, bound=True)
        twin = fbank_host_f32(x, spec)
        assert twin.dtype == np.float32 and twin.shape == M.shape == dM.shape
        err = np.abs(twin.astype(np.float64) - M)
        narrow = ((M > 0) & (dM <= 0.1 * M)) | (M + dM < FLOOR)
        print(f"({win},{hop},{spec.n_fft},{n_mels}) snip {snip}: max err / dM {(err / dM).max():.4f}, dM <= 0.1 M for {narrow.mean():.4f}")
        assert (err <= dM).all()
        assert narrow.mean() >= 0.9                              # what the log-domain check on the device rests on


def test_the_twin_with_every_switch():
    rng = np.random.default_rng(1)
    x = noise(rng, 2, 1500)
    for kw in (dict(remove_dc_offset=False), dict(preemphasis=0.0), dict(use_power=False), dict(scale=1.0), dict(scale=3.3),
               dict(window="hamming"), dict(window="rectangular", remove_dc_offset=False, preemphasis=0.0), dict(snip_edges=False)):
        spec = KaldiFbank(16000, log=False, **kw)
        M, dM = fbank_host(x + np.float32(0.1), spec, bound=True)
        err = np.abs(fbank_host_f32(x + np.float32(0.1), spec).astype(np.float64) - M)
        assert (err <= dM).all(), kw


def test_a_constant_row():
    spec, logged = KaldiFbank(16000, log=False), KaldiFbank(16000)
    x = np.full((1, 3000), 0.3, dtype=np.float32)                # 9830.4 and its sums are not exact in float32
    M, dM = fbank_host(x, spec, bound=True)
    twin = fbank_host_f32(x, spec)
    assert np.abs(M).max() < 1e-12 and (np.abs(twin.astype(np.float64) - M) <= dM).all()
    assert (fbank_host(x, logged) == np.log(FLOOR)).all()
    x = np.full((1, 3000), 0.25, dtype=np.float32)               # 8192: every partial sum is exact, the mean too
    assert (fbank_host_f32(x, spec) == 0).all()
    assert (fbank_host_f32(x, logged) == np.float32(np.log(np.float32(FLOOR)))).all()
    # without the mean's removal the constant is there
    assert fbank_host(x, KaldiFbank(16000, log=False, remove_dc_offset=False)).max() > 1e6


def test_a_nan_reaches_exactly_the_frames_that_contain_it():
    rng = np.random.default_rng(2)
    x = noise(rng, 4000)
    y = x.copy()
    y[1700] = np.nan
    for snip in (True, False):
        spec = KaldiFbank(16000, snip_edges=snip)
        idx = fbank_frame_index(4000, spec)
        hit = (idx == 1700).any(axis=1)
        assert 1 < hit.sum() < 4
        for fn in (fbank_host, fbank_host_f32):
            a, b = fn(x, spec), fn(y, spec)
            assert np.isnan(b[:, hit]).all() and np.array_equal(a[:, ~hit], b[:, ~hit])


def test_refusals_and_immutability():
    good = KaldiFbank(16000)
    assert (good.win_length, good.hop_length, good.n_mels, good.n_fft, good.n_bins) == (400, 160, 80, 512, 257)
    assert good.window.shape == (400,) and good.basis.shape == (400, 514) and good.fb.shape == (80, 257)
    assert all(a.dtype == np.float32 and not a.flags.writeable for a in (good.window, good.basis, good.fb))
    assert good.flags == 15 and KaldiFbank(16000, snip_edges=False, log=False).flags == 6
    assert KaldiFbank(16000, 400, round_to_power_of_two=False).n_fft == 400 and KaldiFbank(16000, 512).n_fft == 512
    with pytest.raises(AttributeError):
        good.n_mels = 3
    with pytest.raises(AttributeError):
        del good.window
    for bad in (dict(sample_rate=0), dict(sample_rate=16000.0), dict(win_length=15), dict(win_length=2049), dict(win_length=400.0),
                dict(hop_length=0), dict(hop_length=401), dict(n_mels=0), dict(n_mels=257), dict(low_freq=-1.0), dict(low_freq=9000.0),
                dict(high_freq=8001.0), dict(high_freq=-7990.0), dict(preemphasis=-0.1), dict(preemphasis=1.5), dict(preemphasis="0.97"),
                dict(preemphasis=float("nan")), dict(remove_dc_offset=1), dict(window="hann"), dict(round_to_power_of_two=None),
                dict(snip_edges="yes"), dict(use_power=0), dict(log="ln"), dict(scale=0.0), dict(scale=float("inf")),
                dict(scale=float("nan")), dict(scale=1e39), dict(scale="1")):
        kw = {"sample_rate": 16000, **bad}
        with pytest.raises(ValueError):
            KaldiFbank(**kw)
    assert KaldiFbank(16000, 2048).n_fft == 2048
    assert KaldiFbank(16000, 1025).n_fft == 2048
    for fn in (fbank_host, fbank_host_f32):
        with pytest.raises(ValueError):
            fn(np.zeros(500, dtype=np.float64), good)
        with pytest.raises(ValueError):
            fn(np.zeros((2, 0), dtype=np.float32), good)
        with pytest.raises(ValueError):
            fn(np.zeros(500, dtype=np.float32), "fbank")
        assert fn(np.zeros((2, 399), dtype=np.float32), good).shape == (2, 80, 0)   # no frame: an empty result


def test_the_package_exports_it():
    import alac.net_amd as pkg

    for name in ("KaldiFbank", "fbank", "fbank_host", "fbank_host_f32", "kaldi_mel_banks"):
        assert hasattr(pkg, name), name
    assert "alacgpu_fbank_device" in pkg.SYMBOLS and hasattr(pkg.AlacGpuContext, "fbank_device")
    # both transforms have what Corpus.crops needs
    for spec in (pkg.LogMel(16000), pkg.KaldiFbank(16000)):
        assert spec.frames(spec.min_frames) >= 1 and str(spec.min_frames - 1) in spec.short(spec.min_frames - 1)
        assert callable(spec.lengths) and callable(spec.launch)
    assert pkg.LogMel(16000).min_frames == 201
