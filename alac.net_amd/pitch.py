"""Pitch shift and time stretch of crops: a phase vocoder (alacgpu_time_stretch_device, csrc/alac_stretch.hip) and, for the
pitch, the resampler without tables behind it (speed.py).

The specification is torchaudio's `phase_vocoder` / `pitch_shift` (`time_stretch_host`, numpy float64, written their way:
angles, wrap, cumsum, np.fft).  A row x[b] float32 [C, T] with v = min(max(lengths[b], 0), T) valid frames is stretched by the
reduced fraction s = p / q, output length over input length; N = n_fft is 512, 1024 or 2048, the hop H = N / 4, the window
w[n] = 0.5 - 0.5 cos(2 pi n / N) (periodic Hann), K = N / 2 + 1 bins.

    STFT      center=True, reflect padding: frame t = 0 .. T_ - 1, T_ = 1 + v div H, is X_t = rfft(w[n] x[refl(t H - N / 2 + n)]),
              refl(i) = -i below 0 and 2 (v - 1) - i from v on.  Two zero frames stand behind them.
    vocoder   output frame j = 0 .. T' - 1, T' = ceil(T_ p / q), reads the frames i = (j q) div p and i + 1 with the weight
              alpha = ((j q) mod p) / p -- integers until that one division:
              |Y_j| = alpha |X_{i+1}| + (1 - alpha) |X_i|,  arg Y_0 = arg X_0,
              arg Y_{j+1} = arg Y_j + wrap(arg X_{i+1} - arg X_i - advance) + advance          (advance = pi H k / (K - 1) of bin k)
    iSTFT     frame j is irfft(Y_j) w; the frames are overlap-added at the hop, the first N / 2 samples dropped, and sample n
              is divided by the envelope, the sum of w^2 of the frames that cover it.  The row gets Ls = (2 v p + q) div (2 q)
              frames (v p / q, half rounded up); sample n is written for n <= (T' - 1) H only, zero from there up to Ls.
              There the envelope is at least 1.25 (1.5 inside).  torch.istft divides by envelopes down to 1e-11 in the last
              N / 2 samples instead: the one stated deviation.

Rows that are left alone, neither read nor written by the kernels: s == 1, v <= N / 2 (no reflection), v <= 0.  Their
new length is their length.

No angle is taken by the kernel.  wrap(d - advance) + advance is d modulo 2 pi and only exp(i cumsum) is used, so with
ph(z) = z / |z|, ph(0) = 1 (torch's angle(0) = 0):

    P_0 = ph(X_0),   P_{j+1} = normalise(P_j * (ph(X_{i+1}) * conj(ph(X_i)))),   Y_j = (alpha |X_{i+1}| + (1 - alpha) |X_i|) P_j

`time_stretch_host(..., phasor=True)` is that form in float64; tests/test_stretch_spec.py holds it to the angle form to 1e-10 of
the row's peak.

The kernel's float32 order, which `time_stretch_host_f32` follows operation for operation -- every operation one IEEE float32
operation, rounded once, nothing fused, division and root the correctly rounded ones:

    analyse     z[n] = (w32[n] * x[refl], 0), n < N, w32 the window computed in float64 and rounded once; an N-point complex
                transform in LDS: for N = 512 and 2048 one radix-2 decimation-in-frequency stage (a + b, (a - b) tw[q] for
                q < N / 2) and then, on both halves, the radix-4 stages of alac_reverb.h of span L = N / 8 .. 1; for 1024 the
                radix-4 stages from L = N / 4.  Twiddles tw[k] = exp(-2 pi i k / N), float64 rounded once.  Bin k is at
                `positions(N)[k]`; the bins 0 .. N / 2 are stored in natural order.
    scan        one lane per (row, channel, bin), j ascending:  |z| = sqrt(x x + y y);  ph(z) = (x / |z|, y / |z|), (1, 0)
                where |z| is not above 0;  alpha = float(jq mod p) / float(p);
                mag = alpha * |X_{i+1}| + (1 - alpha) * |X_i|;  Y_j = (mag * P.x, mag * P.y);
                d = ph(X_{i+1}) * conj(ph(X_i));  t = P_j * d;  P_{j+1} = ph(t)      (a complex product is
                (ar br - ai bi, ar bi + ai br)); frames at and behind T_ are zero.
    synthesise  frame j: the spectrum of N points is Y_j[k] at positions(N)[k] for k <= N / 2 (the imaginary parts of the
                bins 0 and N / 2 dropped, as irfft does) and its conjugate at positions(N)[N - k]; the inverse stages in the
                opposite order; c_j[i] = w32[i] * (re z[i] * (1 / N)).  Sample n: acc = 0 + c_j[n + N / 2 - j H] over the
                frames 0 <= j < T' that cover it in ascending j, env = 0 + w32[i] * w32[i] likewise, y[n] = acc / env.

The bound, derived, not measured (`time_stretch_host(..., bound=True)` returns it per element).  u = 2^-24, gamma_k = k u /
(1 - k u).  The transform: as in reverb.py, a radix-4 stage is two radix-2 stages of which one has exact twiddles, so Higham's
Theorem 24.2 for log2 N radix-2 stages covers it: the computed transform of z is within f sqrt(N) ||z||_2 in the 2-norm,
f = s eta / (1 - s eta), s = log2 N, eta = u + gamma_4 (sqrt(2) + u).  The windowed frame carries 2 u + u^2 of its elements (the
window's rounding and the product's), so every bin of frame t is within

    e_t = (f + (2 u + u^2)(1 + f)) sqrt(N) ||w x_t||_2

of the specification's X_t[k].  The magnitude: ||a'| - |a|| <= |a' - a|, the root of a sum of squares adds 2 u, alpha, 1 - alpha,
the two products and the sum one rounding each: dmag <= (1 + 8 u)(alpha e_{i+1} + (1 - alpha) e_i) + 8 u mag.  The phasor:
|ph(a') - ph(a)| <= 2 |a' - a| / |a| for any a', and its own root and division add 4 u; a step of the chain adds the errors
of its two phasors, two complex products at sqrt(2) gamma_2 each and the normalisation's 4 u, together 24 u to first order,
so the drift is linear in j:

    dP_0 = 2 e_0 / |X_0| + 4 u,    dP_{j+1} = dP_j + 2 e_i / |X_i| + 2 e_{i+1} / |X_{i+1}| + 24 u,    both capped at 2

(two unit vectors are never further apart; a bin of magnitude 0 has the cap: its phase is not determined, and a bin that is
small in one frame keeps what it lost there -- the phase vocoder's own condition, not the arithmetic's).  Then
dY_j[k] = dmag + (mag + dmag)(dP_j + 2 u).  The inverse transform of a frame is linear: an element of it moves by at most
(1 / N) sum over the N bins of dY_j (the bins 1 .. N / 2 - 1 count twice), and the transform's own rounding adds
f ||Y_j||_2 / sqrt(N) (1 + ...) per element: E_j = (1 / N) sum dY_j + f (||Y_j||_2 + ||dY_j||_2) / sqrt(N).  The four terms of
the overlap-add are each a product with w32 (2 u) and added in float32 (gamma_3); the envelope is a float32 sum of four rounded
squares of rounded weights, within gamma_8 of the true one, and the division adds u:

    dy[n] = (1 + 16 u) (sum over the frames j that cover n of w[i] E_j) / env[n] + 16 u (sum of |w[i] c_j[i]|) / env[n]

It assumes that nothing underflows and is first order in u.  It is loose by design -- the cap of 2 stands for every bin that
is ever small --; tests/test_stretch_spec.py prints the share of it that the twin uses.

The stages.  Specification, twin and bound are each three functions that `vocoder_host` and `vocoder_host_f32` compose:

    analyse      x -> X [C, T_ + 2, K]       `analyse_host`      `analyse_host_f32`       `analyse_bound`      e_t, 2-norm of a frame
    scan         X, p, q -> Y [C, T', K]     `scan_host`         `scan_host_f32`          `scan_bound`         dY per element
    synthesise   Y, v, p, q -> y [C, Ls]     `synthesise_host`   `synthesise_host_f32`    `synthesise_bound`   dy per sample

(`scan_host` is the phasor form, `scan_host(..., phasor=False)` the angles; the twins take and give (real, imaginary) pairs of
float32 arrays; `hermitian_host_f32` is the copy that lays Y out as the spectra of N points in front of the inverse transform.)
A stage's bound is how far its float32 evaluation may be from its float64 one on the same, exact input: the formulas above
with the incoming error at zero --

    analyse      e_t as above
    scan         dmag = 8 u mag + u alpha |X_i|,  dP_0 = 4 u,  dP_{j+1} = dP_j + 24 u,  dY = dmag + (mag + dmag)(dP + 2 u)
    synthesise   E_j = f ||Y_j||_2 / sqrt(N),  dy[n] as above

-- and `vocoder_host(..., bound=True)` is the three fed into each other (`scan_bound(e=)`, `synthesise_bound(dY=)`).  The
condition of the vocoder sits in that feeding, in e / |X|, not in any stage, so the stage bounds are tight where the
end-to-end one cannot be: tests/test_stretch_stages.py holds every stage of the twin to them (profiles/stretch_stages.json).
The term u alpha |X_i| is one the end-to-end derivation lacks: alpha is a rounded quotient, off by u alpha, and 1 - alpha
inherits that absolutely, not relative to itself, so (1 - alpha) |X_i| is off by u alpha |X_i| -- which 8 u mag does not cover
where alpha is near 1 and |X_{i+1}| small (the zero frames behind the last one, terms up to 2^20).  `scan_bound` has it;
`vocoder_host(..., bound=True)` returns what it always has, without it: there (mag + dmag) dP is larger by orders of magnitude
on every row that has been measured, but that is an observation, not part of the derivation.

Pitch shift by the ratio rho = p / q: stretch by rho, then play rho times faster through speed.py's resampler, unchanged:
the ratio a : b = p : q, new length ceil(q Ls / p); the first min(v, new length) frames are written and zeros behind them up
to v; lengths stay and what lies behind them is not touched.  `pitch_shift_host` composes `time_stretch_host` with
`speed_host`, `pitch_shift_host_f32` the twins.  Semitones become ratios on the host: Fraction(2 ** (n / 12))
.limit_denominator(200), within 0.03 cents of the equal-tempered interval for |n| <= 2 and within 1.96 cents for |n| <= 12
(the worst is -7 semitones, 2 / 3; `cents_error`).

`PitchShift`, the host functions and `positions` need no device.  `time_stretch` and `pitch_shift` are the calls on device
tensors; `Corpus.crops(pitch=)` runs the pitch shift behind the waveform and `speed=` and in front of `reverb=`.
Out of scope: tempo perturbation inside `crops` (it changes the source window, as speed= does; `time_stretch` on the result
covers it), formant preservation, identity phase locking, n_fft outside 512 / 1024 / 2048, hops other than n_fft / 4.
"""
import math
from fractions import Fraction

import numpy as np

from ._stageargs import _lengths_device, _lengths_host, _planes, _span, _Spec, _device_context, _f32_finite
from .speed import _factor, ratio as _speed_ratio, speed_host, speed_host_f32

_U = 2.0 ** -24
N_FFTS = (512, 1024, 2048)
MAX_SEMITONE_DENOMINATOR = 200


# ---- the integers ----------------------------------------------------------------------------------------------------------------
def _n_fft(n_fft):
    if isinstance(n_fft, (bool, np.bool_)) or not isinstance(n_fft, (int, np.integer)) or int(n_fft) not in N_FFTS:
        raise ValueError(f"n_fft must be one of {N_FFTS}, not {n_fft!r}")
    return int(n_fft)


def stft_frames(v, n_fft):
    """T_ = 1 + v div hop"""
    return 1 + v // (n_fft // 4)


def vocoder_frames(T, p, q):
    """T' = ceil(T p / q)"""
    return -(-T * p // q)


def stretched_frames(v, p, q):
    """Ls = (2 v p + q) div (2 q): v p / q, half rounded up"""
    return (2 * v * p + q) // (2 * q)


def steps(T, p, q):
    """(i, num) for j < T': output frame j reads the frames i[j] and i[j] + 1 with alpha = num[j] / p"""
    j = np.arange(vocoder_frames(T, p, q), dtype=np.int64)
    return (j * q) // p, (j * q) % p


def live(v, p, q, n_fft):
    """Whether a row of v valid frames at the factor p / q is stretched at all"""
    return p != q and v > n_fft // 2


def window(n_fft, dtype=np.float64):
    """The periodic Hann window, computed in float64 (and rounded once for float32)"""
    return (0.5 - 0.5 * np.cos(2.0 * 3.14159265358979323846 * np.arange(n_fft, dtype=np.float64) / float(n_fft))).astype(dtype)


def twiddles(n_fft):
    """The kernel's table: (cos, -sin)(2 pi k / N), k < N, computed in float64 and rounded once to float32"""
    a = 2.0 * 3.14159265358979323846 * np.arange(n_fft, dtype=np.float64) / float(n_fft)
    return np.cos(a).astype(np.float32), (-np.sin(a)).astype(np.float32)


def _radix(n_fft):
    """(whether a radix-2 stage leads, the radix-4 digits behind it)"""
    bits = n_fft.bit_length() - 1
    return bits % 2 == 1, bits // 2


def positions(n_fft):
    """Where bin k < N of the kernel's forward transform lies: the base-4 digits of k reversed, for 512 and 2048 of k div 2 in
    the half that k mod 2 names"""
    odd, digits = _radix(n_fft)
    k = np.arange(n_fft, dtype=np.int64)
    kk = k >> 1 if odd else k
    rev = np.zeros_like(k)
    for _ in range(digits):
        rev = rev * 4 + (kk & 3)
        kk = kk >> 2
    return (k & 1) * (n_fft // 2) + rev if odd else rev


def _reflect(v, n_fft, T):
    """[T, N]: the frame of x that element n of STFT frame t reads"""
    i = (np.arange(T, dtype=np.int64) * (n_fft // 4))[:, None] - n_fft // 2 + np.arange(n_fft, dtype=np.int64)[None, :]
    i = np.where(i < 0, -i, i)
    return np.where(i >= v, 2 * (v - 1) - i, i)


# ---- the policy -----------------------------------------------------------------------------------------------------------------
def semitone_ratio(n):
    """The ratio of n semitones as a reduced fraction of a denominator of at most 200"""
    n = _f32_finite("a semitone count", n)
    return Fraction(2.0 ** (n / 12.0)).limit_denominator(MAX_SEMITONE_DENOMINATOR)


def cents_error(n):
    """How far `semitone_ratio(n)` is from n equal-tempered semitones, in cents"""
    return 1200.0 * math.log2(float(semitone_ratio(n))) - 100.0 * float(n)


class PitchShift(_Spec):
    """The policy: a crop's pitch is changed by one of `ratios`, drawn with the probabilities `weights` (default: uniform), and
    with probability 1 - p by the ratio 1 whatever was drawn.  semitones: numbers, each becoming `semitone_ratio(n)`:
    Fraction(2 ** (n / 12)).limit_denominator(200), within 1.96 cents for |n| <= 12 (-2 .. 2: 49/55 .. 55/49, within 0.03 cents);
    or ratios=: ints, Fractions or floats read by their decimal repr, as speed.SpeedPerturb's factors, instead.  `ratios` is the
    tuple the draws index: the given ones as Fractions and 1 behind them if it is not among them; `one` is the index of 1.
    n_fft: 512, 1024 or 2048.  Immutable.  ValueError: a ratio outside 1/2 .. 2 or with a denominator above 1000, an empty
    list, a duplicate, both semitones and ratios, weights that are not as many non-negative finite numbers with a positive sum,
    p outside 0 .. 1, another n_fft."""

    __slots__ = ("ratios", "weights", "p", "n_fft")

    def __init__(self, semitones=(-2, -1, 0, 1, 2), ratios=None, weights=None, p=1.0, n_fft=512):
        try:
            if ratios is not None:
                if tuple(semitones) != (-2, -1, 0, 1, 2):
                    raise ValueError("give semitones or ratios, not both")
                given = tuple(_factor(v) for v in ratios)
            else:
                given = tuple(_factor(semitone_ratio(v)) for v in semitones)
        except TypeError:
            raise ValueError(f"semitones and ratios must be sequences of numbers, not {semitones!r} and {ratios!r}") from None
        if not given:
            raise ValueError("semitones or ratios must not be empty")
        if len(set(given)) != len(given):
            raise ValueError(f"{given!r} has a duplicate")
        if weights is None:
            w = (1.0,) * len(given)
        else:
            try:
                w = tuple(_f32_finite("a weight", v, least=0.0) for v in weights)
            except TypeError:
                raise ValueError(f"weights must be a sequence of numbers, not {weights!r}") from None
            if len(w) != len(given) or not sum(w) > 0:
                raise ValueError(f"weights must be {len(given)} non-negative numbers with a positive sum, not {weights!r}")
        p = _f32_finite("p", p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be in 0 .. 1, not {p!r}")
        s = object.__setattr__
        s(self, "ratios", given if Fraction(1) in given else given + (Fraction(1),))
        s(self, "weights", w + (0.0,) * (len(self.ratios) - len(w)))
        s(self, "p", p)
        s(self, "n_fft", _n_fft(n_fft))

    @property
    def one(self):
        return self.ratios.index(Fraction(1))

    def draw(self, B, generator=None, device="cuda"):
        """Indices into `ratios` for B crops: an int64 tensor [B] on `device`, by torch operations only; nothing is read back.
        Two draws of B float64 uniforms each, in this order: u, the ratio -- the first index whose cumulative weight, as a
        share of the sum, is above u --, then v: the crop keeps its ratio if v < p, else it gets `one`.  generator: a
        torch.Generator of that device or of the CPU (the draws are then made there and uploaded)."""
        import torch

        here = torch.device(device)
        dev = generator.device if generator is not None else here
        cum = np.cumsum(np.asarray(self.weights, dtype=np.float64))
        edges = torch.from_numpy(cum[:-1] / cum[-1]).to(here)
        u = torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here)
        v = torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here)
        k = torch.searchsorted(edges, u, right=True).clamp(max=len(self.ratios) - 1)
        return torch.where(v < self.p, k, self.one).to(torch.int64)


# ---- the specification ----------------------------------------------------------------------------------------------------------
def _host_args(x, factors, lengths, n_fft):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 3 or x.shape[1] == 0:
        raise ValueError(f"x must be float32 [B, C, T], not {x.dtype} {x.shape}")
    B, C, T = x.shape
    many = isinstance(factors, (list, tuple, np.ndarray))
    fs = [_factor(f) for f in factors] if many else [_factor(factors)] * B
    if len(fs) != B:
        raise ValueError(f"{len(fs)} factors for {B} rows")
    return x, fs, _lengths_host("lengths", lengths, B, T), _n_fft(n_fft)


def _fft_factor(n_fft):
    """f of the module docstring: the relative 2-norm error of the float32 transform"""
    gam = lambda k: k * _U / (1 - k * _U)
    eta = _U + gam(4) * (math.sqrt(2.0) + _U)
    s = n_fft.bit_length() - 1
    return s * eta / (1 - s * eta)


def _windowed(xr, n_fft):
    """[C, T_, N] float64: the reflected, windowed frames of xr [C, v]"""
    xr = np.asarray(xr, dtype=np.float64)
    v = xr.shape[1]
    if v <= n_fft // 2:
        raise ValueError(f"{v} frames cannot be reflected by {n_fft // 2}")
    return xr[:, _reflect(v, n_fft, stft_frames(v, n_fft))] * window(n_fft)


def analyse_host(xr, n_fft):
    """The analysis stage in float64: xr float32 or float64 [C, v], v > n_fft / 2, to X complex128 [C, T_ + 2, K], the STFT
    frames and the two zero frames behind them"""
    frames = _windowed(xr, n_fft)                                               # [C, T, N]
    C, T, _ = frames.shape
    X = np.zeros((C, T + 2, n_fft // 2 + 1), dtype=np.complex128)
    X[:, :T] = np.fft.rfft(frames, axis=-1)
    return X


def analyse_bound(xr, n_fft):
    """e [C, T_ + 2]: how far, in the 2-norm over a frame's bins, a float32 `analyse_host_f32` of an exact xr may be from
    `analyse_host` (e_t of the module docstring; 0 for the two zero frames)"""
    frames = _windowed(xr, n_fft)
    C, T, N = frames.shape
    f = _fft_factor(N)
    e = np.zeros((C, T + 2))
    e[:, :T] = (f + (2 * _U + _U * _U) * (1 + f)) * math.sqrt(N) * np.sqrt((frames ** 2).sum(axis=-1))
    return e


def _scan_parts(X, p, q):
    """(i, alpha [1, T', 1], a = X_i, b = X_{i + 1}, mag) of X [C, T_ + 2, K]"""
    X = np.asarray(X, dtype=np.complex128)
    i, num = steps(X.shape[1] - 2, p, q)
    alpha = (num.astype(np.float64) / float(p))[None, :, None]
    a, b = X[:, i], X[:, i + 1]
    return i, alpha, a, b, alpha * np.abs(b) + (1.0 - alpha) * np.abs(a)


def scan_host(X, p, q, phasor=True):
    """The scan stage in float64: X complex [C, T_ + 2, K] to Y complex128 [C, T', K]; the phasor form, or (phasor=False)
    torchaudio's angles"""
    X = np.asarray(X, dtype=np.complex128)
    C, _, K = X.shape
    i, alpha, a, b, mag = _scan_parts(X, p, q)
    Tp = len(i)
    if phasor:
        ph = lambda z: np.where(np.abs(z) > 0, z / np.where(np.abs(z) > 0, np.abs(z), 1.0), 1.0)
        d = ph(b) * np.conj(ph(a))
        P = np.empty((C, Tp, K), dtype=np.complex128)
        P[:, 0] = ph(X[:, 0])
        for j in range(Tp - 1):
            P[:, j + 1] = ph(P[:, j] * d[:, j])
        return mag * P
    advance = np.linspace(0.0, math.pi * ((K - 1) // 2), K)[None, None, :]
    phase = np.angle(b) - np.angle(a) - advance
    phase = phase - 2.0 * math.pi * np.round(phase / (2.0 * math.pi))
    phase = phase + advance
    phase = np.concatenate([np.angle(X[:, :1]), phase[:, :-1]], axis=1)
    return mag * np.exp(1j * np.cumsum(phase, axis=1))


def scan_bound(X, p, q, e=None, alpha_term=True):
    """dY [C, T', K]: how far a float32 `scan_host_f32` may be from `scan_host`, per element.  e: None for an exact X (the
    stage's own bound: dmag = 8 u mag + u alpha |X_i|, dP_0 = 4 u, dP_{j+1} = dP_j + 24 u), or [C, T_ + 2], how far every bin
    of a frame of the X it got may be from this one.  alpha_term: the u alpha |X_i| of the module docstring (`vocoder_host`
    leaves it out, as it always has)."""
    X = np.asarray(X, dtype=np.complex128)
    C, _, K = X.shape
    i, alpha, a, b, mag = _scan_parts(X, p, q)
    Tp = len(i)
    if e is None:
        e = np.zeros((C, X.shape[1]))
    ea, eb = e[:, i][:, :, None], e[:, i + 1][:, :, None]
    dmag = (1 + 8 * _U) * (alpha * eb + (1 - alpha) * ea) + 8 * _U * mag
    if alpha_term:
        dmag = dmag + _U * alpha * np.abs(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        turn = lambda err, z: np.where(err > 0, np.minimum(2.0 * err / np.abs(z), 2.0), 0.0)
        step = turn(ea, a) + turn(eb, b) + 24 * _U
        dP = np.empty((C, Tp, K))
        dP[:, 0] = np.minimum(turn(e[:, 0][:, None], X[:, 0]) + 4 * _U, 2.0)
        for j in range(Tp - 1):
            dP[:, j + 1] = np.minimum(dP[:, j] + step[:, j], 2.0)
    return dmag + (mag + dmag) * (dP + 2 * _U)


def _overlap_add(Y, v, p, q, dY=None):
    """What `synthesise_host` and `synthesise_bound` share: (y [C, Ls], dy [C, Ls] or None) of Y complex [C, T', K]"""
    Y = np.asarray(Y, dtype=np.complex128)
    C, Tp, K = Y.shape
    N = 2 * (K - 1)
    H = N // 4
    w = window(N)
    fr = np.fft.irfft(Y, n=N, axis=-1) * w                                      # [C, T', N]
    Ls = stretched_frames(v, p, q)
    total = (Tp - 1) * H + N
    acc, env, absacc = np.zeros((C, total)), np.zeros(total), np.zeros((C, total))
    for j in range(Tp):
        acc[:, j * H:j * H + N] += fr[:, j]
        absacc[:, j * H:j * H + N] += np.abs(fr[:, j])
        env[j * H:j * H + N] += w * w
    n = min(Ls, (Tp - 1) * H + 1)
    y = np.zeros((C, Ls))
    y[:, :n] = acc[:, N // 2:N // 2 + n] / env[N // 2:N // 2 + n]
    if dY is None:
        return y, None
    f = _fft_factor(N)
    twice = np.full(K, 2.0)
    twice[0] = twice[-1] = 1.0
    norm = lambda z: np.sqrt((twice * z * z).sum(axis=-1))
    E = (twice * dY).sum(axis=-1) / N + f * (norm(np.abs(Y)) + norm(dY)) / math.sqrt(N)        # [C, T']
    eacc = np.zeros((C, total))
    for j in range(Tp):
        eacc[:, j * H:j * H + N] += w * E[:, j][:, None]
    dy = np.zeros((C, Ls))
    s = slice(N // 2, N // 2 + n)
    dy[:, :n] = ((1 + 16 * _U) * eacc[:, s] + 16 * _U * absacc[:, s]) / env[s]
    return y, dy


def synthesise_host(Y, v, p, q):
    """The synthesis stage in float64: Y complex [C, T', K] of a row of v valid frames at p / q to y float64 [C, Ls]"""
    return _overlap_add(Y, v, p, q)[0]


def synthesise_bound(Y, v, p, q, dY=None):
    """dy [C, Ls]: how far a float32 `synthesise_host_f32` may be from `synthesise_host`, per sample.  dY: None for an exact
    Y (the stage's own bound: E_j = f ||Y_j||_2 / sqrt(N)), or [C, T', K], how far every element of the Y it got may be from
    this one."""
    Y = np.asarray(Y, dtype=np.complex128)
    return _overlap_add(Y, v, p, q, np.zeros(Y.shape) if dY is None else dY)[1]


def vocoder_host(xr, p, q, n_fft, phasor=False, bound=False):
    """One row through the vocoder in float64, whatever p / q is (1 too): xr float32 or float64 [C, v], v > n_fft / 2, to
    float64 [C, Ls]: `analyse_host`, `scan_host`, `synthesise_host`.  phasor: the phasor form instead of torchaudio's angles.
    bound=True: returns (y, dy), dy how far a float32 evaluation in the kernel's order may be from y (the module docstring):
    the three stage bounds, each fed the one before."""
    v = np.shape(xr)[1]
    X = analyse_host(xr, n_fft)
    Y = scan_host(X, p, q, phasor=phasor)
    if not bound:
        return synthesise_host(Y, v, p, q)
    return _overlap_add(Y, v, p, q, scan_bound(X, p, q, analyse_bound(xr, n_fft), alpha_term=False))


def _rows(x, factors, lengths, n_fft, row, dtype):
    """What the four host functions share: every live row through row(x[b, :, :v], p, q, N) -> [C, Ls]; the others copied.
    Returns (y [B, C, max new length], new lengths int64 [B])"""
    x, fs, v, N = _host_args(x, factors, lengths, n_fft)
    B, C, T = x.shape
    news = np.array([stretched_frames(int(v[b]), f.numerator, f.denominator) if live(int(v[b]), f.numerator, f.denominator, N)
                     else int(v[b]) for b, f in enumerate(fs)], dtype=np.int64)
    y = np.zeros((B, C, int(news.max()) if B else 0), dtype=dtype)
    with np.errstate(all="ignore"):
        for b, f in enumerate(fs):
            k = int(v[b])
            if live(k, f.numerator, f.denominator, N):
                y[b, :, :news[b]] = row(x[b, :, :k], f.numerator, f.denominator, N)
            else:
                y[b, :, :k] = x[b, :, :k]
    return y, news


def time_stretch_host(x, factors, lengths=None, n_fft=512, phasor=False, bound=False):
    """The specification in numpy float64: x float32 [B, C, T] stretched by `factors` (one factor or B: ints, Fractions or
    floats read by their decimal repr, 1/2 .. 2) to (y float64 [B, C, max new length], new lengths int64 [B]); zeros behind a
    row's new length.  lengths: [B] integers (default T).  phasor: the phasor form.  bound=True: (y, new lengths, dy)."""
    if not bound:
        return _rows(x, factors, lengths, n_fft, lambda xr, p, q, N: vocoder_host(xr, p, q, N, phasor=phasor), np.float64)
    dys = []

    def row(xr, p, q, N):
        y, dy = vocoder_host(xr, p, q, N, phasor=phasor, bound=True)
        dys.append(dy)
        return y

    y, news = _rows(x, factors, lengths, n_fft, row, np.float64)
    dY = np.zeros_like(y)
    x_, fs, v, N = _host_args(x, factors, lengths, n_fft)
    it = iter(dys)
    for b, f in enumerate(fs):
        if live(int(v[b]), f.numerator, f.denominator, N):
            dY[b, :, :news[b]] = next(it)
    return y, news, dY


# ---- the float32 twin -------------------------------------------------------------------------------------------------------------
def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1]), (a[0] * b[1] + a[1] * b[0])


def _butterflies(N, L):
    q = np.arange(N // 4)
    j = q & (L - 1)
    i0 = ((q - j) << 2) + j
    step = N // (4 * L)
    return (i0, i0 + L, i0 + 2 * L, i0 + 3 * L), (j * step, 2 * j * step, 3 * j * step)


def _forward(zr, zi, tw):
    """The kernel's forward transform of [n, N] float32 (real and imaginary parts) in place; bin k ends at positions(N)[k]"""
    N = zr.shape[1]
    odd, _ = _radix(N)
    L = N // 4
    if odd:
        h = N // 2
        a, b = (zr[:, :h].copy(), zi[:, :h].copy()), (zr[:, h:].copy(), zi[:, h:].copy())
        zr[:, :h], zi[:, :h] = a[0] + b[0], a[1] + b[1]
        zr[:, h:], zi[:, h:] = _cmul((a[0] - b[0], a[1] - b[1]), (tw[0][:h], tw[1][:h]))
        L = N // 8
    while L >= 1:
        (i0, i1, i2, i3), ks = _butterflies(N, L)
        a, b, c, d = ((zr[:, i], zi[:, i]) for i in (i0, i1, i2, i3))
        t0, t1, t2 = (a[0] + c[0], a[1] + c[1]), (a[0] - c[0], a[1] - c[1]), (b[0] + d[0], b[1] + d[1])
        bd = (b[0] - d[0], b[1] - d[1])
        t3 = (bd[1], -bd[0])
        outs = ((t0[0] + t2[0], t0[1] + t2[1]), (t1[0] + t3[0], t1[1] + t3[1]), (t0[0] - t2[0], t0[1] - t2[1]), (t1[0] - t3[0], t1[1] - t3[1]))
        zr[:, i0], zi[:, i0] = outs[0]
        for i, o, k in zip((i1, i2, i3), outs[1:], ks):
            zr[:, i], zi[:, i] = _cmul(o, (tw[0][k], tw[1][k]))
        L //= 4


def _inverse(zr, zi, tw):
    """The kernel's inverse transform, not divided by N: the forward stages' conjugate transposes in the opposite order"""
    N = zr.shape[1]
    odd, _ = _radix(N)
    L = 1
    while L <= (N // 8 if odd else N // 4):
        (i0, i1, i2, i3), ks = _butterflies(N, L)
        z0 = (zr[:, i0], zi[:, i0])
        z1, z2, z3 = (_cmul((zr[:, i], zi[:, i]), (tw[0][k], -tw[1][k])) for i, k in zip((i1, i2, i3), ks))
        u0, u1, u2 = (z0[0] + z2[0], z0[1] + z2[1]), (z0[0] - z2[0], z0[1] - z2[1]), (z1[0] + z3[0], z1[1] + z3[1])
        dz = (z1[0] - z3[0], z1[1] - z3[1])
        u3 = (-dz[1], dz[0])
        outs = ((u0[0] + u2[0], u0[1] + u2[1]), (u1[0] + u3[0], u1[1] + u3[1]), (u0[0] - u2[0], u0[1] - u2[1]), (u1[0] - u3[0], u1[1] - u3[1]))
        for i, o in zip((i0, i1, i2, i3), outs):
            zr[:, i], zi[:, i] = o
        L *= 4
    if odd:
        h = N // 2
        a = (zr[:, :h].copy(), zi[:, :h].copy())
        b = _cmul((zr[:, h:], zi[:, h:]), (tw[0][:h], -tw[1][:h]))
        zr[:, :h], zi[:, :h] = a[0] + b[0], a[1] + b[1]
        zr[:, h:], zi[:, h:] = a[0] - b[0], a[1] - b[1]


def _abs32(z):
    return np.sqrt(z[0] * z[0] + z[1] * z[1])


def _ph32(z):
    m = _abs32(z)
    ok = m > 0
    safe = np.where(ok, m, np.float32(1))
    return np.where(ok, z[0] / safe, np.float32(1)).astype(np.float32), np.where(ok, z[1] / safe, np.float32(0)).astype(np.float32)


def analyse_host_f32(xr, n_fft):
    """The kernel's analysis in numpy float32: xr float32 [C, v], v > n_fft / 2, to X = (Xr, Xi), float32 [C, T_ + 2, K] each,
    the STFT frames and the two zero frames behind them"""
    f32 = np.float32
    xr = np.asarray(xr, dtype=f32)
    C, v = xr.shape
    N, K = n_fft, n_fft // 2 + 1
    w, tw, pos = window(N, f32), twiddles(N), positions(N)
    T = stft_frames(v, N)
    zr = np.ascontiguousarray((w * xr[:, _reflect(v, N, T)]).reshape(C * T, N), dtype=f32)
    zi = np.zeros_like(zr)
    _forward(zr, zi, tw)
    Xr, Xi = np.zeros((C, T + 2, K), dtype=f32), np.zeros((C, T + 2, K), dtype=f32)
    Xr[:, :T], Xi[:, :T] = zr[:, pos[:K]].reshape(C, T, K), zi[:, pos[:K]].reshape(C, T, K)
    return Xr, Xi


def scan_host_f32(X, p, q):
    """The kernel's scan in numpy float32: X = (Xr, Xi) float32 [C, T_ + 2, K] to Y = (Yr, Yi), float32 [C, T', K] each"""
    f32 = np.float32
    Xr, Xi = X
    C, T2, K = Xr.shape
    i, num = steps(T2 - 2, p, q)
    Tp = len(i)
    alpha = num.astype(f32) / f32(p)
    Yr, Yi = np.zeros((C, Tp, K), dtype=f32), np.zeros((C, Tp, K), dtype=f32)
    P = _ph32((Xr[:, 0], Xi[:, 0]))
    for j in range(Tp):
        a, b = (Xr[:, i[j]], Xi[:, i[j]]), (Xr[:, i[j] + 1], Xi[:, i[j] + 1])
        mag = alpha[j] * _abs32(b) + (f32(1) - alpha[j]) * _abs32(a)
        Yr[:, j], Yi[:, j] = mag * P[0], mag * P[1]
        pa, pb = _ph32(a), _ph32(b)
        P = _ph32(_cmul(P, _cmul(pb, (pa[0], -pa[1]))))
    return Yr, Yi


def hermitian_host_f32(Y):
    """The spectra of N points the kernel's inverse transform starts from: Y = (Yr, Yi) float32 [C, T', K] to (zr, zi) float32
    [C T', N]: Y_j[k] at positions(N)[k] for k <= N / 2, the imaginary parts of the bins 0 and N / 2 dropped, and its conjugate
    at positions(N)[N - k].  A copy: no arithmetic."""
    f32 = np.float32
    Yr, Yi = Y
    C, Tp, K = Yr.shape
    N = 2 * (K - 1)
    pos = positions(N)
    zr, zi = np.zeros((C * Tp, N), dtype=f32), np.zeros((C * Tp, N), dtype=f32)
    zr[:, pos[:K]] = Yr.reshape(C * Tp, K)
    zi[:, pos[1:K - 1]] = Yi.reshape(C * Tp, K)[:, 1:K - 1]
    mirror = pos[N - np.arange(1, K - 1)]
    zr[:, mirror] = Yr.reshape(C * Tp, K)[:, 1:K - 1]
    zi[:, mirror] = -Yi.reshape(C * Tp, K)[:, 1:K - 1]
    return zr, zi


def synthesise_host_f32(Y, v, p, q):
    """The kernel's synthesis in numpy float32: Y = (Yr, Yi) float32 [C, T', K] of a row of v valid frames at p / q to y
    float32 [C, Ls]"""
    f32 = np.float32
    Yr, Yi = Y
    C, Tp, K = Yr.shape
    N = 2 * (K - 1)
    H = N // 4
    w, tw = window(N, f32), twiddles(N)
    zr, zi = hermitian_host_f32(Y)
    _inverse(zr, zi, tw)
    fr = (w * (zr * f32(1.0 / N))).reshape(C, Tp, N)
    total = (Tp - 1) * H + N
    acc, env = np.zeros((C, total), dtype=f32), np.zeros(total, dtype=f32)
    w2 = w * w
    for j in range(Tp):
        acc[:, j * H:j * H + N] += fr[:, j]
        env[j * H:j * H + N] += w2
    Ls = stretched_frames(v, p, q)
    n = min(Ls, (Tp - 1) * H + 1)
    y = np.zeros((C, Ls), dtype=f32)
    y[:, :n] = acc[:, N // 2:N // 2 + n] / env[N // 2:N // 2 + n]
    return y


def vocoder_host_f32(xr, p, q, n_fft):
    """One row through the kernel's scheme in numpy float32, operation for operation (the module docstring): xr float32
    [C, v], v > n_fft / 2, to float32 [C, Ls]: `analyse_host_f32`, `scan_host_f32`, `synthesise_host_f32`"""
    v = np.shape(xr)[1]
    return synthesise_host_f32(scan_host_f32(analyse_host_f32(xr, n_fft), p, q), v, p, q)


def time_stretch_host_f32(x, factors, lengths=None, n_fft=512):
    """The kernel's float32 twin: as `time_stretch_host`, to (y float32 [B, C, max new length], new lengths).  The kernel
    equals it bit for bit."""
    return _rows(x, factors, lengths, n_fft, vocoder_host_f32, np.float32)


def _pitch_rows(x, ratios, rate, lengths, n_fft, stretch, resample, dtype):
    x, fs, v, N = _host_args(x, ratios, lengths, n_fft)
    s, news = stretch(x, fs, v, N)
    y = x.astype(dtype)
    for b, f in enumerate(fs):
        k = int(v[b])
        if live(k, f.numerator, f.denominator, N):
            a, bb, width = _speed_ratio(rate, f, rate)
            y[b, :, :k] = resample(s[b, :, :news[b]], a, bb, width, num_frames=k)
    return y


def pitch_shift_host(x, ratios, rate, lengths=None, n_fft=512):
    """The specification of the pitch shift: `time_stretch_host` by the ratios, then `speed.speed_host` at them: float64
    [B, C, T], x itself behind the lengths and in the rows that are left alone"""
    return _pitch_rows(x, ratios, rate, lengths, n_fft, time_stretch_host, speed_host, np.float64)


def pitch_shift_host_f32(x, ratios, rate, lengths=None, n_fft=512):
    """The float32 twin of the pitch shift: `time_stretch_host_f32`, then `speed.speed_host_f32`.  The calls on the device
    equal it bit for bit."""
    return _pitch_rows(x, ratios, rate, lengths, n_fft, time_stretch_host_f32, speed_host_f32, np.float32)


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _fractions_device(fs, device):
    import torch

    pq = np.array([[f.numerator, f.denominator] for f in fs], dtype=np.int32).reshape(-1, 2)
    return torch.from_numpy(np.ascontiguousarray(pq[:, 0])).to(device), torch.from_numpy(np.ascontiguousarray(pq[:, 1])).to(device)


def time_stretch(x, factors, lengths=None, n_fft=512):
    """Time stretch on the GPU, the pitch kept: x float32 [B, C, T] on the device, contiguous or the slice [..., :T] of a
    contiguous tensor (what lies behind the slice is not read), stretched by `factors` (one factor or B: ints, Fractions or
    floats read by their decimal repr, 1/2 .. 2; above 1 is longer and slower).  Returns (y float32 [B, C, max new length],
    new lengths int64 [B] on the device): row b has (2 v p + q) div (2 q) frames, zeros behind them; a row at factor 1 or of
    at most n_fft / 2 valid frames is copied.  lengths: [B] integers, a sequence or a tensor (read back to size y; -1 counts as
    0, more than T as T).  Three launches, asynchronous on the current stream; ValueError before any device work."""
    import torch

    ctx = _device_context("x", x, "[B, C, T]")
    S = _planes("x", x)
    B, C, T = x.shape
    N = _n_fft(n_fft)
    many = isinstance(factors, (list, tuple, np.ndarray))
    fs = [_factor(f) for f in factors] if many else [_factor(factors)] * B
    if len(fs) != B:
        raise ValueError(f"{len(fs)} factors for {B} rows")
    if isinstance(lengths, torch.Tensor):
        d_valid = _lengths_device("lengths", lengths, B, x.device)
        v = np.clip(d_valid.cpu().numpy(), 0, T)
    else:
        v = _lengths_host("lengths", lengths, B, T)
        d_valid = _lengths_device("lengths", lengths, B, x.device)
    alone = np.array([not live(int(v[b]), f.numerator, f.denominator, N) for b, f in enumerate(fs)], dtype=bool)
    news = np.array([int(v[b]) if alone[b] else stretched_frames(int(v[b]), f.numerator, f.denominator) for b, f in enumerate(fs)],
                    dtype=np.int64)
    Lo = int(news.max()) if B else 0
    y = torch.empty((B, C, Lo), dtype=torch.float32, device=x.device)
    new_lengths = torch.from_numpy(news).to(x.device)
    if B == 0 or Lo == 0:
        return y, new_lengths
    if alone.any():             # the rows the kernels leave alone: their valid frames, zeros behind them
        rows = torch.from_numpy(np.nonzero(alone)[0]).to(x.device)
        n = min(T, Lo)
        keep = torch.arange(n, device=x.device)[None, None, :] < new_lengths[rows][:, None, None]
        y[rows] = 0
        y[rows, :, :n] = torch.where(keep, x[rows, :, :n], torch.zeros((), dtype=x.dtype, device=x.device))
    if not alone.all():
        d_p, d_q = _fractions_device(fs, x.device)
        d_new = torch.empty(B, dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device).cuda_stream
            ctx().time_stretch_device(x, y, B, C, S, Lo, T, Lo, d_p, d_q, d_valid, d_new, N, stream=stream)
    return y, new_lengths


def _pitch_shift(ctx, x, d_p, d_q, ratios, d_row_ratio, lengths, n_fft, out, scratch):
    """`pitch_shift` behind its checks, for device-side ratios: d_p, d_q int32 [B] (1, 1 where a row is left alone), `ratios`
    the resampler's uint32 [kinds, 3] with a = 0 for the ratio 1 and d_row_ratio int32 [B] the kind of every row (a kind with
    a = 0, or len(ratios), where a row is left alone).  scratch(name, shape) gives a float32 device tensor of that shape that
    the caller keeps; Ls_max = scratch's frames.  ctx() gives the context that runs it."""
    import torch

    S = _planes("x", x)
    B, C, T = x.shape
    N = n_fft
    So = _planes("out", out)
    most = max(float(Fraction(int(a), int(b))) if a else 1.0 for a, b, _ in ratios)
    Lmax = max(int(math.floor(T * most + 0.5)) + 1, 1)
    stretched = scratch("stretched", (B, C, Lmax))
    resampled = scratch("resampled", (B, C, T))
    d_valid = lengths if lengths is not None else torch.full((B,), T, dtype=torch.int64, device=x.device)
    d_new = torch.empty(B, dtype=torch.int64, device=x.device)
    d_ratios = torch.from_numpy(np.ascontiguousarray(ratios).view(np.int32)).to(x.device)
    zeros = torch.zeros(B, dtype=torch.int64, device=x.device)
    # the rows the vocoder stretches are the rows the resampler and the copy take: the others keep x
    is_live = (d_p != d_q) & (d_valid > N // 2)
    row_ratio = torch.where(is_live, d_row_ratio, len(ratios)).to(torch.int32)
    placed = torch.where(is_live, d_valid.clamp(max=T), 0)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        c = ctx()
        c.time_stretch_device(x, stretched, B, C, S, Lmax, T, Lmax, d_p, d_q, d_valid, d_new, N, stream=stream)
        c.resample_ratio_rows_device(stretched, B, C, Lmax, zeros, d_new, zeros, T, ratios, d_ratios, row_ratio, False, resampled, stream=stream)
        c.copy_rows_device(resampled, out, B, C, T, So, T, placed, stream=stream)
    return out


def _ratio_kinds(fs, rate):
    """The resampler's kinds of a list of ratios: (uint32 [kinds, 3] of (a, b, width), a = 0 for the ratio 1; the kind of each)"""
    kinds = []
    for f in fs:
        a, b, width = _speed_ratio(rate, f, rate)
        kinds.append((0, 1, 1) if f == 1 else (a, b, width))
    return np.asarray(kinds, dtype=np.uint32).reshape(-1, 3)


def checked_rate(rate):
    if isinstance(rate, (bool, np.bool_)) or not isinstance(rate, (int, np.integer)) or int(rate) <= 0:
        raise ValueError(f"rate must be a positive integer, not {rate!r}")
    return int(rate)


def pitch_shift(x, ratios, rate, lengths=None, n_fft=512, out=None):
    """Pitch shift on the GPU, the duration kept: x float32 [B, C, T] on the device, C 1 or 2, contiguous or the slice
    [..., :T] of a contiguous tensor; row b's pitch is multiplied by ratios[b] (one ratio or B: ints, Fractions or floats read
    by their decimal repr, 1/2 .. 2; `semitone_ratio` gives a semitone count's).  rate: the sample rate of x, an integer (the
    resampler's filter depends on the ratio alone).  lengths: [B] integers, a sequence or a tensor (-1 counts as 0, more than
    T as T): a row's first v frames are replaced, what lies behind them is neither read nor written; a row at the ratio 1 or
    of at most n_fft / 2 valid frames is left as it is, bit for bit.  out: x itself (in place) or a tensor of x's shape and
    layout apart from it (it then gets a copy of x first); default: a new one.  Returns out.  Bit for bit
    `speed_perturb(time_stretch(x, ratios, lengths, n_fft), ratios, rate, rate, new lengths)` cropped to the lengths.  Five
    launches, asynchronous on the current stream, nothing read back; ValueError before any device work."""
    import torch

    ctx = _device_context("x", x, "[B, C, T]")
    S = _planes("x", x)
    B, C, T = x.shape
    if C not in (1, 2):
        raise ValueError(f"{C} channels: the resampler takes 1 or 2")
    N = _n_fft(n_fft)
    rate = checked_rate(rate)
    many = isinstance(ratios, (list, tuple, np.ndarray))
    fs = [_factor(f) for f in ratios] if many else [_factor(ratios)] * B
    if len(fs) != B:
        raise ValueError(f"{len(fs)} ratios for {B} rows")
    if out is not None and out is not x:
        if (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
                or (x.numel() and _planes("out", out) != S)):
            raise ValueError("out must be x itself or a float32 tensor of x's shape, layout and device")
        if x.numel():
            (x0, x1), (o0, o1) = _span(x, S), _span(out, S)
            if x0 < o1 and o0 < x1:
                raise ValueError("out overlaps x without being x")
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    d_valid = _lengths_device("lengths", lengths, B, x.device)
    if out is None:
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    if x.numel() == 0:
        return out
    if out is not x:
        out.copy_(x)            # (what the stage leaves untouched is x's)
    kinds, index = [], {}
    for f in fs:
        index.setdefault(f, len(index))
    kinds = _ratio_kinds(list(index), rate)
    d_p, d_q = _fractions_device(fs, x.device)
    d_row = torch.from_numpy(np.array([index[f] for f in fs], dtype=np.int32)).to(x.device)
    held = {}

    def scratch(name, shape):
        held[name] = torch.empty(shape, dtype=torch.float32, device=x.device)
        return held[name]

    return _pitch_shift(ctx, x, d_p, d_q, kinds, d_row, d_valid, N, out, scratch)
