"""The phase vocoder's specification and its float32 twin, without a device (alac.net_amd/pitch.py): the phasor form against
torchaudio's angles, the identity at factor 1, what a stretch and a pitch shift do to a sine, the envelope, the integers
against independent big-integer formulas, the policy's refusals and semitone fractions, the header and the bindings, and the
twin held to the specification within the bound the module derives."""
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (F(200, 189), F(9, 10), F(2), F(1, 2), F(11, 10))


@pytest.fixture(scope="module")
def pitch():
    import alac.net_amd.pitch as m

    return m


def signal(seed, C, T, rate=16000):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    x = 0.2 * rng.standard_normal((C, T)) + 0.5 * np.sin(2 * np.pi * 330.0 * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t))
    return x.astype(np.float32)


def test_the_phasor_form_is_the_angle_form(pitch):
    for n_fft, T in ((512, 4000), (1024, 3000), (2048, 5000)):
        x = signal(n_fft, 2, T)
        for f in FACTORS:
            a = pitch.vocoder_host(x, f.numerator, f.denominator, n_fft)
            b = pitch.vocoder_host(x, f.numerator, f.denominator, n_fft, phasor=True)
            worst = np.abs(a - b).max() / np.abs(a).max()
            print(f"n_fft {n_fft} factor {f}: phasor form {worst:.3g} of the peak from the angle form")
            assert a.shape == b.shape == (2, pitch.stretched_frames(T, f.numerator, f.denominator))
            assert worst <= 1e-10


def test_factor_one_through_the_vocoder_is_the_identity(pitch):
    for n_fft in pitch.N_FFTS:
        H = n_fft // 4
        for T in (n_fft // 2 + 1, 3 * n_fft + 17, 8 * H):
            x = signal(T, 1, T)
            y, dy = pitch.vocoder_host(x, 1, 1, n_fft, bound=True)
            n = min((pitch.stft_frames(T, n_fft) - 1) * H + 1, T)     # the samples n <= (T_ - 1) H
            assert y.shape == (1, T) and T - n < H
            assert np.abs(y[:, :n] - x[:, :n]).max() <= 1e-10 * np.abs(x).max()
            assert not y[:, n:].any()
            y32 = pitch.vocoder_host_f32(x, 1, 1, n_fft)
            assert (np.abs(y32 - y) <= dy).all()


def test_a_sine_at_a_bin_centre_keeps_its_frequency_when_stretched(pitch):
    n_fft, T, k = 512, 6000, 20
    x = np.sin(2 * np.pi * k / n_fft * np.arange(T)).astype(np.float32)[None, None]
    y, lens = pitch.time_stretch_host(x, F(3, 2))
    assert lens.tolist() == [9000] and y.shape == (1, 1, 9000)
    seg = y[0, 0, 1024:1024 + 8 * n_fft] * np.hanning(8 * n_fft)
    peak = int(np.argmax(np.abs(np.fft.rfft(seg))))
    assert peak == 8 * k                                    # the same frequency in a finer grid
    assert 0.5 < np.abs(y[0, 0, 1024:8000]).max() < 1.5        # (no phase locking: the three bins of the sine keep the phases of frame 0)


def test_a_pitch_shift_moves_the_spectral_peak_and_keeps_the_length(pitch):
    rate, T, f0 = 16000, 8000, 500.0
    x = np.sin(2 * np.pi * f0 / rate * np.arange(T)).astype(np.float32)[None, None]
    for rho in (F(55, 49), F(49, 55), F(4, 3)):
        y = pitch.pitch_shift_host(x, rho, rate, lengths=[7000])
        assert y.shape == x.shape and np.array_equal(y[0, 0, 7000:], x[0, 0, 7000:].astype(np.float64))
        n = 4096
        spec = np.abs(np.fft.rfft(y[0, 0, 1024:1024 + n] * np.hanning(n)))
        got = np.argmax(spec) * rate / n
        assert abs(got - float(rho) * f0) <= rate / n, (rho, got)
        # the twin likewise (a pure sine leaves most bins at rounding level, whose phases are not determined: the two differ
        # where the reflected end lights those bins up, within the bound; test_the_twin_is_within_the_derived_bound... holds that)
        y32 = pitch.pitch_shift_host_f32(x, rho, rate, lengths=[7000])
        spec32 = np.abs(np.fft.rfft(y32[0, 0, 1024:1024 + n].astype(np.float64) * np.hanning(n)))
        assert np.argmax(spec32) == np.argmax(spec) and np.array_equal(y32[0, 0, 7000:], x[0, 0, 7000:])
        assert np.abs(y32 - y)[0, 0, :4000].max() < 1e-4


def test_the_envelope_over_the_written_samples(pitch):
    for n_fft in pitch.N_FFTS:
        H, w = n_fft // 4, pitch.window(n_fft)
        for frames in (2, 3, 4, 9):                          # (a live row has at least 3 STFT frames and, at 1/2, 2 output frames)
            env = np.zeros((frames - 1) * H + n_fft)
            for j in range(frames):
                env[j * H:j * H + n_fft] += w * w
            written = env[n_fft // 2:n_fft // 2 + (frames - 1) * H + 1]
            print(f"n_fft {n_fft}, {frames} frames: envelope {written.min():.6f} .. {written.max():.6f}")
            assert written.min() >= 1.25 - 1e-12 and written.max() <= 1.5 + 1e-12
        assert abs(env[n_fft]) - 1.5 < 1e-12
        w32 = pitch.window(n_fft, np.float32)
        assert w32.dtype == np.float32 and w32[0] == 0 and w32[n_fft // 2] == 1 and np.array_equal(w32[1:], w32[:0:-1])


def test_the_integers_against_big_integer_formulas(pitch):
    rng = np.random.default_rng(7)
    for _ in range(300):
        n_fft = int(rng.choice(pitch.N_FFTS))
        v = int(rng.integers(n_fft // 2 + 1, 1 << 40))
        f = F(int(rng.integers(1, 1001)), int(rng.integers(1, 1001)))
        if not F(1, 2) <= f <= 2:
            continue
        p, q = f.numerator, f.denominator
        T = v // (n_fft // 4) + 1
        assert pitch.stft_frames(v, n_fft) == T
        assert pitch.vocoder_frames(T, p, q) == math.ceil(F(T) * f)
        assert pitch.stretched_frames(v, p, q) == math.floor(F(v) * f + F(1, 2))
    for T, f in ((3, F(1, 2)), (17, F(200, 189)), (40, F(2)), (33, F(9, 10)), (12, F(11, 10))):
        p, q = f.numerator, f.denominator
        i, num = pitch.steps(T, p, q)
        assert len(i) == math.ceil(F(T) * f)
        for j in range(len(i)):
            t = F(j) / f                                    # torchaudio's time step: j * rate, rate = 1 / factor
            assert i[j] == math.floor(t) and F(int(num[j]), p) == t - math.floor(t)
        assert i[-1] + 1 <= T + 1                           # the two zero frames suffice
    for n_fft in pitch.N_FFTS:
        pos = pitch.positions(n_fft)
        assert sorted(pos.tolist()) == list(range(n_fft))
        z = np.random.default_rng(n_fft).standard_normal((2, n_fft)).astype(np.float32)
        zr, zi = z.copy(), np.zeros_like(z)
        pitch._forward(zr, zi, pitch.twiddles(n_fft))
        ref = np.fft.fft(z.astype(np.float64))
        assert np.abs((zr[:, pos] + 1j * zi[:, pos]) - ref).max() <= pitch._fft_factor(n_fft) * np.sqrt(n_fft) * np.linalg.norm(z, axis=1).max()
        pitch._inverse(zr, zi, pitch.twiddles(n_fft))
        assert np.abs(zr / n_fft - z).max() < 1e-5 and np.abs(zi).max() / n_fft < 1e-5


def test_rows_that_are_left_alone_and_the_lengths(pitch):
    x = np.stack([signal(b, 2, 1500) for b in range(5)])
    lengths = [-1, 256, 257, 1500, 900]
    factors = [F(9, 10), F(9, 10), F(9, 10), 1, 1.1]
    y, lens = pitch.time_stretch_host(x, factors, lengths)
    assert lens.tolist() == [0, 256, 231, 1500, 990] and y.shape == (5, 2, 1500)
    assert np.array_equal(y[1, :, :256], x[1, :, :256].astype(np.float64)) and not y[1, :, 256:].any()
    assert np.array_equal(y[3], x[3].astype(np.float64)) and not y[0].any() and not y[2, :, 231:].any()
    y32, lens32 = pitch.time_stretch_host_f32(x, factors, lengths)
    assert lens32.tolist() == lens.tolist() and np.array_equal(y32[3], x[3]) and y32.dtype == np.float32
    for bad in (lambda: pitch.time_stretch_host(x, factors[:4], lengths), lambda: pitch.time_stretch_host(x, 3), lambda: pitch.time_stretch_host(x, F(1, 1001)),
                lambda: pitch.time_stretch_host(x, 1.1, n_fft=256), lambda: pitch.time_stretch_host(x.astype(np.float64), 1.1),
                lambda: pitch.time_stretch_host(x, 1.1, lengths=[1.5] * 5), lambda: pitch.pitch_shift_host(x, 1.1, 16000.0)):
        with pytest.raises(ValueError):
            bad()


def test_the_policy(pitch):
    spec = pitch.PitchShift()
    assert spec.ratios == (F(49, 55), F(185, 196), F(1), F(196, 185), F(55, 49)) and spec.one == 2 and spec.n_fft == 512
    assert spec.weights == (1.0,) * 5 and spec == pitch.PitchShift() and hash(spec) == hash(pitch.PitchShift())
    for n in range(-12, 13):
        r = pitch.semitone_ratio(n)
        assert r == F(2.0 ** (n / 12.0)).limit_denominator(200) and r.denominator <= 200 and F(1, 2) <= r <= 2
        assert abs(pitch.cents_error(n)) < 2.0 and (abs(n) > 2 or abs(pitch.cents_error(n)) < 0.03)
        assert abs(1200 * math.log2(float(r)) - 100 * n - pitch.cents_error(n)) < 1e-9
    other = pitch.PitchShift(ratios=(0.9, F(11, 10)), weights=(1, 3), p=0.5, n_fft=2048)
    assert other.ratios == (F(9, 10), F(11, 10), F(1)) and other.weights == (1.0, 3.0, 0.0) and other.one == 2
    with pytest.raises(AttributeError):
        spec.p = 0.5
    for bad in (dict(semitones=()), dict(semitones=(1, 1)), dict(semitones=(13,)), dict(semitones=("a",)), dict(semitones=5),
                dict(ratios=(3,)), dict(ratios=(F(1, 1001) + 1,)), dict(ratios=(1.1,), semitones=(1,)), dict(weights=(1, 2)),
                dict(weights=(0,) * 5), dict(weights=(-1, 1, 1, 1, 1)), dict(p=1.5), dict(p=float("nan")), dict(n_fft=256), dict(n_fft=512.0)):
        with pytest.raises(ValueError):
            pitch.PitchShift(**bad)


def test_the_header_and_the_bindings_declare_the_entry_points():
    import alac.net_amd as pkg

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alacgpu.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    for name, n_args in (("alacgpu_time_stretch_device", 15), ("alacgpu_copy_rows_device", 10)):
        m = re.search(name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == n_args, f"{name} is not declared in include/alacgpu.h with {n_args} arguments"
        assert len(pkg.SYMBOLS[name][1]) == n_args
        m = re.search(r"extern int " + name + r"\(([^)]*)\)", cs)
        assert m and len(m.group(1).split(",")) == n_args, f"{name} in AlacGpuNative.cs"
    for name in ("PitchShift", "pitch_shift", "time_stretch", "pitch_shift_host", "pitch_shift_host_f32", "time_stretch_host",
                 "time_stretch_host_f32"):
        assert hasattr(pkg, name)


def test_the_twin_is_within_the_derived_bound_of_the_specification(pitch):
    """The worst share of the bound the twin uses is printed; the bound is pitch.py's, derived there."""
    worst = 0.0
    for n_fft, T, C in ((512, 4000, 2), (1024, 3000, 1), (2048, 5000, 1)):
        x = np.stack([signal(10 * n_fft + b, C, T) for b in range(len(FACTORS))])
        lengths = [T, T - 77, T // 2 + 100, T - 1, n_fft // 2 + 1]
        y, lens, dy = pitch.time_stretch_host(x, list(FACTORS), lengths, n_fft, bound=True)
        y32, lens32 = pitch.time_stretch_host_f32(x, list(FACTORS), lengths, n_fft)
        assert lens.tolist() == lens32.tolist() and y32.shape == y.shape and np.isfinite(dy).all()
        err = np.abs(y32.astype(np.float64) - y)
        assert (err <= dy).all()
        share = (err[dy > 0] / dy[dy > 0]).max()
        peak = np.abs(y).max()
        print(f"n_fft {n_fft}: the twin is within {err.max():.3g} of the specification (peak {peak:.3g}), at most {share:.3g} of the bound; "
              f"the bound is at most {dy.max():.3g}")
        worst = max(worst, share)
        assert dy.max() < peak                              # loose, but it says something
    print(f"worst share of the bound: {worst:.3g}")
    assert 0 < worst <= 1
