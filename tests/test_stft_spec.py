"""alac.net_amd/stft.py without a device: the float32 twin against the float64 specification inside the derived bound, the
bound against two wrong evaluations, the specification against `logmel_host`, the properties of the pairing, the constructor's
refusals and `as_complex`."""
import numpy as np
import pytest

SR = 16000


def noise(L, seed, rows=2):
    """Rows of full-scale uniform noise"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, L)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def custom_window(n):
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * (np.arange(n) + 0.5) / n)).astype(np.float32)


def cases(pkg):
    out = {}
    for N in (256, 512, 1024, 2048):
        for power in (2, 1, None):
            out[f"n_fft {N}, power {power}"] = (dict(n_fft=N, power=power), 2 * N + 77)
    mel = pkg.mel_filterbank(SR, 512, 40)
    for log in ("ln", "log10", None):
        out[f"mel, log {log}"] = (dict(n_fft=512, hop_length=160, filterbank=mel, log=log), 2100)
    out["mel of the magnitude, ln"] = (dict(n_fft=512, hop_length=160, power=1, filterbank=mel, log="ln"), 2100)
    out["win_length 400 in 512"] = (dict(n_fft=512, hop_length=160, win_length=400), 2000)
    out["an odd win_length"] = (dict(n_fft=256, hop_length=100, win_length=201, power=1), 1500)
    out["a custom window"] = (dict(n_fft=256, hop_length=64, win_length=200, window=custom_window(200), power=None), 1400)
    return out


def test_the_twin_is_inside_the_bound_of_the_specification():
    import alac.net_amd as pkg

    for i, (name, (kw, L)) in enumerate(cases(pkg).items()):
        spec = pkg.Spectrogram(SR, **kw)
        x = noise(L, 10 + i)
        ref, bound = pkg.spectrogram_host(x, spec, bound=True)
        twin = pkg.spectrogram_host_f32(x, spec)
        T = 1 + L // spec.hop_length
        assert ref.shape == twin.shape == bound.shape == (2, spec.n_mels, T) and twin.dtype == np.float32, name
        err = np.abs(twin.astype(np.float64) - ref)
        rel = np.median(bound / np.maximum(np.abs(ref), 1e-300))
        print(f"{name}: worst error / bound {float((err / bound).max()):.3g}, the bound's median relative size {float(rel):.3g}")
        assert np.isfinite(twin).all() and (bound > 0).all() and (err <= bound).all(), name
        assert rel < 2e-3, name                       # (a bound of a few 1e-4 of the value: it says something)


@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048])
def test_the_bound_is_not_vacuous(n_fft):
    """One twiddle off by 2^-12 -- table[0], which every stage multiplies by -- and the pair unpacked with a wrong sign both
    leave it"""
    import alac.net_amd as pkg
    from alac.net_amd import pitch

    for power in (2, None):
        spec = pkg.Spectrogram(SR, n_fft, power=power)
        x = noise(3 * n_fft, n_fft + (power or 0))
        ref, bound = pkg.spectrogram_host(x, spec, bound=True)
        cos, msin = (t.copy() for t in pitch.twiddles(n_fft))
        cos[0] += np.float32(2.0 ** -12)
        off = pkg.spectrogram_host_f32(x, spec, table=(cos, msin))
        flipped = pkg.spectrogram_host_f32(x, spec, unpack_sign=-1.0)
        for name, wrong in (("a twiddle off by 2^-12", off), ("a wrong sign in the unpacking", flipped)):
            outside = np.abs(wrong.astype(np.float64) - ref) > bound
            print(f"n_fft {n_fft}, power {power}, {name}: {int(outside.sum())} of {outside.size} elements leave the bound")
            assert outside.any(), (power, name)


def test_the_specification_agrees_with_logmel_host():
    """The same mel configuration at n_fft 512 by both modules: the margin is the sum of their own bounds (both in the power
    domain, where `logmel_host` states its bound)"""
    import alac.net_amd as pkg

    x = noise(4000, 3)
    lm = pkg.LogMel(SR, 512, 160, 80, log=None)
    a, da = pkg.logmel_host(x, lm, bound=True)
    spec = pkg.Spectrogram(SR, 512, 160, filterbank=pkg.mel_filterbank(SR, 512, 80))
    b, db = pkg.spectrogram_host(x, spec, bound=True)
    assert a.shape == b.shape and (np.abs(a - b) <= da + db).all()
    print(f"worst difference / margin {float((np.abs(a - b) / (da + db)).max()):.3g}")
    # and behind the log: the two logs are of values that close
    la = pkg.logmel_host(x, pkg.LogMel(SR, 512, 160, 80, log="ln"))
    lb, dlb = pkg.spectrogram_host(x, pkg.Spectrogram(SR, 512, 160, filterbank=pkg.mel_filterbank(SR, 512, 80), log="ln"), bound=True)
    assert (np.abs(la - lb) <= dlb + da / np.maximum(a, 1e-10) * 1.001 + 1e-12).all()


def test_the_pairing_is_by_parity_and_a_frame_reads_its_own_taps_only():
    import alac.net_amd as pkg

    for power in (2, None):
        spec = pkg.Spectrogram(SR, 256, 64, power=power)
        x = noise(64 * 9 + 10, 5, rows=1)
        odd = pkg.spectrogram_host_f32(x, spec)                          # 10 frames ...
        assert odd.shape[-1] == 10
        # T' odd and even: the frames they share, but those whose taps reach the end (they reflect about another L)
        longer = np.concatenate([x, noise(64, 6, rows=1)], axis=1)     # ... 11 frames: frame 10 is a lone one
        more = pkg.spectrogram_host_f32(longer, spec)
        assert more.shape[-1] == 11
        inside = [t for t in range(10) if t * 64 + 128 <= x.shape[1]]
        assert len(inside) >= 7 and np.array_equal(bits(odd[..., inside]), bits(more[..., inside]))
        # a frame's bits do not depend on L beyond its own taps, nor on its partner's samples
        other = longer.copy()
        other[0, 64 * 5 + 128:] = noise(other.shape[1] - (64 * 5 + 128), 7, rows=1)[0]      # behind frame 5's last tap
        changed = pkg.spectrogram_host_f32(other, spec)
        assert np.array_equal(bits(changed[..., :4]), bits(more[..., :4]))                  # the pairs (0, 1) and (2, 3): whole
        assert not np.array_equal(bits(changed[..., 6:]), bits(more[..., 6:]))
        # (frame 4 shares its transform with frame 5, whose samples changed: within the bound, not bit for bit)
        ref, bound = pkg.spectrogram_host(other, spec, bound=True)
        assert (np.abs(changed - ref) <= bound).all()


def test_what_is_not_finite_stays_in_its_pair():
    import alac.net_amd as pkg

    spec = pkg.Spectrogram(SR, 256, 64, power=1)
    x = noise(64 * 12, 8, rows=1)
    clean = pkg.spectrogram_host_f32(x, spec)
    for value in (np.nan, np.inf):
        y = x.copy()
        y[0, 64 * 6] = value                    # the centre of frame 6: a tap of the frames 5 .. 8 (of 8 the first, of weight zero)
        got = pkg.spectrogram_host_f32(y, spec)
        touched = [4, 5, 6, 7, 8, 9]            # the pairs (4, 5), (6, 7) and (8, 9)
        rest = [t for t in range(got.shape[-1]) if t not in touched]
        assert len(rest) == 7 and np.array_equal(bits(got[..., rest]), bits(clean[..., rest]))
        assert not np.isfinite(got[..., [5, 6, 7, 8]]).all(axis=1).any()
        assert not np.isfinite(got[..., 4]).all() and not np.isfinite(got[..., 9]).all()      # no tap on it: their partners have


def test_the_constructor_refuses():
    import alac.net_amd as pkg

    fb = pkg.mel_filterbank(SR, 512, 40)
    ok = pkg.Spectrogram(SR, 512, filterbank=fb, log="ln")
    assert ok.n_mels == 40 and ok.hop_length == 128 and ok.win_length == 512 and ok.n_bins == 257 and ok.min_frames == 257
    assert pkg.Spectrogram(SR).n_mels == 513 and pkg.Spectrogram(SR, power=None).n_mels == 1026
    for kw in (dict(n_fft=400), dict(n_fft=128), dict(n_fft=4096), dict(n_fft=512.0), dict(n_fft=True), dict(hop_length=0),
               dict(hop_length=1025), dict(hop_length=2.5), dict(win_length=0), dict(win_length=1025), dict(power=3), dict(power=0),
               dict(power=True), dict(power="2"), dict(log="log2"), dict(floor=0.0), dict(floor=float("inf")), dict(floor=float("nan")),
               dict(floor=1e-60), dict(window=np.ones(1023, np.float32)), dict(window=np.full(1024, np.nan, np.float32)),
               dict(win_length=400, window=np.ones(1024, np.float32)), dict(filterbank=np.ones((3, 512), np.float32)),
               dict(filterbank=np.ones((257, 513), np.float32)), dict(filterbank=np.ones((0, 513), np.float32)),
               dict(filterbank=np.ones(513, np.float32)), dict(filterbank=np.full((2, 513), np.inf, np.float32)),
               dict(power=None, log="ln"), dict(power=None, filterbank=np.ones((3, 513), np.float32))):
        with pytest.raises(ValueError):
            pkg.Spectrogram(SR, **kw)
    with pytest.raises(ValueError):
        pkg.Spectrogram(0)
    with pytest.raises(AttributeError):
        ok.n_fft = 256
    with pytest.raises(ValueError):
        ok.window[0] = 1.0
    for bad in (np.zeros(256, np.float32), np.zeros(600), np.float32(1.0)):
        with pytest.raises(ValueError):
            pkg.spectrogram_host(bad, ok)
        with pytest.raises(ValueError):
            pkg.spectrogram_host_f32(bad, ok)


def test_the_filterbank_tables():
    import alac.net_amd as pkg

    fb = np.zeros((5, 129), dtype=np.float32)
    fb[0, 7] = 2.0                                   # a band of one bin
    fb[2] = 0.25                                     # a dense row; row 1 is zeros
    fb[3, 120:] = 1.0                                # a band that ends at the Nyquist bin
    fb[4, [3, 9]] = -1.0, 1.0                        # zeros inside a band
    spec = pkg.Spectrogram(SR, 256, filterbank=fb)
    assert spec.bands.tolist() == [[7, 1, 0], [0, 0, 1], [0, 129, 1], [120, 9, 130], [3, 7, 139]]
    assert len(spec.weights) == 147 and spec.weights[0] == 2.0 and spec.weights[139] == -1.0 and spec.weights[145] == 1.0
    x = noise(1000, 9)
    got = pkg.spectrogram_host_f32(x, spec)
    ref, bound = pkg.spectrogram_host(x, spec, bound=True)
    assert not got[:, 1].any() and (np.abs(got - ref) <= bound).all()
    logged = pkg.spectrogram_host_f32(x, pkg.Spectrogram(SR, 256, filterbank=fb[:4], log="ln", floor=1e-3))
    assert (logged[:, 1] == np.float32(np.log(np.float64(np.float32(1e-3))))).all()


def test_as_complex():
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import stft

    spec = pkg.Spectrogram(SR, 256, power=None)
    x = noise(700, 11)
    feats = torch.from_numpy(pkg.spectrogram_host_f32(x, spec))
    z = stft.as_complex(feats)
    assert z.dtype == torch.complex64 and z.shape == (2, 129, feats.shape[-1])
    assert torch.equal(z.real, feats[:, :129]) and torch.equal(z.imag, feats[:, 129:])
    want = torch.stft(torch.from_numpy(x), 256, 64, window=torch.from_numpy(np.array(spec.window)), center=True, pad_mode="reflect",
                      return_complex=True)
    assert torch.allclose(z, want, atol=2e-4, rtol=0)
    for bad in (feats.numpy(), feats.double(), feats[:, :257], feats[0, 0]):
        with pytest.raises(ValueError):
            stft.as_complex(bad)


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_the_transform_is_the_phase_vocoders(n_fft):
    """The bits of the twin's transform are those of `pitch.analyse_host_f32` on a real frame with a zero partner"""
    import alac.net_amd as pkg
    from alac.net_amd import pitch, stft

    x = noise(3 * n_fft, n_fft, rows=1)
    Xr, Xi = pitch.analyse_host_f32(x, n_fft)                              # [1, T + 2, K]
    T = Xr.shape[1] - 2
    spec = pkg.Spectrogram(SR, n_fft)                                       # the same hop, the same window
    assert np.array_equal(spec.window, pitch.window(n_fft, np.float32))
    idx, inside = pkg.features.frame_index(x.shape[1], n_fft, n_fft // 4)
    assert inside.all() and idx.shape[0] == T
    fr = x[0][idx] * spec.window
    Zr, Zi = stft.transform_host_f32(fr, np.zeros_like(fr))
    K = n_fft // 2 + 1
    assert np.array_equal(bits(Zr[:, :K]), bits(Xr[0, :T])) and np.array_equal(bits(Zi[:, :K]), bits(Xi[0, :T]))
