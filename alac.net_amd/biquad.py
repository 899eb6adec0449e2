"""Biquad filters and a gain on the waveform, behind the noise and in front of the features (alacgpu_biquad_device,
csrc/alac_biquad.hip): volume perturbation, band-limiting and the random EQ of the augmentation libraries are all "a cascade
of second-order IIR sections and a gain per crop".

A row is a crop x[b] float32 [C, T] with v = min(max(lengths[b], 0), T) (T without lengths), its coefficients q[b] float64
[S, 5] = (b0, b1, b2, a1, a2) with a0 divided out, 1 <= S <= 8, and a gain g[b] float64.  With u_0 = x widened exactly to
float64 and every section starting from zero history, for n < v

    u_{k+1}[n] = b0 u_k[n] + b1 u_k[n-1] + b2 u_k[n-2] - a1 u_{k+1}[n-1] - a2 u_{k+1}[n-2]      float64, left to right
    y[c, n]    = fl32(g * u_S[n])                                                               rounded once

with `clamp` then min(max(y, -1), 1), a NaN staying a NaN.  Frames at or behind v are untouched, and a row whose sections are
all exactly (1, 0, 0, 0, 0) with a gain of exactly 1 and no clamp is neither read nor written: "this crop draws nothing".
`biquad_host` is this in numpy, sample after sample.  Float32 is not enough inside the recurrence: a 20 Hz high-pass at 48 kHz
has a recursive impulse response of L1 norm 1.6e5, and float32 direct-form arithmetic is then wrong by a per cent of the peak.

The kernel's order (csrc/alac_biquad.h), which `biquad_host_twin` follows operation by operation, nothing fused: a workgroup
of THREADS = 256 lanes takes a (row, channel) in tiles of TILE = 4096 frames, lane l the CHUNK = 16 frames from 16 l on.  Per
section, with in = (u_k[n0 - 1], u_k[n0 - 2]) in front of the lane's chunk (zeros in front of the row):
    w[j]  = (b0 u[j] + b1 u[j-1]) + b2 u[j-2]                        the FIR part
    y0[j] = (w[j] - a1 y0[j-1]) - a2 y0[j-2],  y0[-1] = y0[-2] = 0   the zero-state recursion; z = (y0[15], y0[14])
    h1, h2: the section's two homogeneous responses over a chunk, g[j] = (-(a1 g[j-1])) - (a2 g[j-2]) from (g[-1], g[-2]) =
        (1, 0) and (0, 1), run once per row and section; M = [[h1[15], h2[15]], [h1[14], h2[14]]] advances a state (y[n-1],
        y[n-2]) by a chunk, and P_0 = M, P_{i+1} = P_i P_i (each element (p q) + (p' q'), row times column) by 2^i chunks
    the states z are combined within a wave of 64 lanes by an inclusive scan, s = (P_i t) + s for the lanes >= 2^i, t the s
        of the lane 2^i below, i = 0 .. 5, a product P t being ((p00 t0) + (p01 t1), (p10 t0) + (p11 t1))
    the state c_w in front of wave w: c_0 the state carried from the tile before (zeros for the first), c_{w+1} = (P_6 c_w) + s
        of lane 63 of wave w; c_4 is carried to the next tile
    e = M^l c_w + s of the lane below, M^l c_w as q = c_w, then q = P_i q for every set bit i of l in ascending order, and e =
        q for lane 0 of a wave: the state in front of the lane's chunk
    u_{k+1}[j] = (y0[j] + h1[j] e0) + h2[j] e1, and e is the next section's `in`
and y = fl32(g u_S) behind the last section.  Every order is fixed, so the same inputs give the same bits, and the result
does not depend on the width of the loads.

The bound D on |blocked - sequential| (`biquad_host(..., bound=True)`), for stable sections, u = 2^-53.  Every rounding error
is an error injected into a sample or into a state at a lane's boundary, and what it does to a later sample is the section's
own exact linear map of it, whatever the order the sums were formed in: an error d in sample m moves sample n by r[n - m] d, r
the recursive impulse response, and an error of norm d in a state moves a sample or a state n frames on by at most Hs[n] d,
Hs[n] = max(|r[n]| + |a2 r[n-1]|, |r[n-1]| + |a2 r[n-2]|) the row-sum norm of the n-th power of the transition matrix.  The
specification computes, per section, over the T frames of a row: G = sum |r[n]|, R = max(1, max Hs), GH = max over j < 16 of
the sum over q of Hs[16 q + j] (what the errors injected at every lane boundary add up to in one place), and with
Bf = |b0| + |b1| + |b2|, Af = |a1| + |a2|, Um = max |u_k|, Ym = max |u_{k+1}| the magnitudes.  In exact arithmetic a zero-state
response over any span is the true response minus the homogeneous response of the true state in front of it, so every partial
state of the scan and every y0 is at most Sm = (1 + R) Ym.  The tables are measured, not bounded: dP = the largest row-sum
norm of P_i - M^(2^i) and dh = max |h1 - exact| + |h2 - exact|, the exact values by integer arithmetic on the coefficients.
    sequential, 9 rounded quantities of at most Q = Bf Um + Af Ym a sample:        E' = G (Bf E + 9 u Q)
    blocked, the FIR's 5 and the recursion's 4 a sample, propagated like any input:  G (Bf E + u (5 Bf Um + 4 (Bf Um + Af Sm)))
      a scan operation (4 rounded quantities of at most (R + 1) Sm, the table's error times Sm):  es = (4 u (R + 1) + dP) Sm
      7 of them at a boundary that later lanes read (6 levels and the wave's carry), 7 more of the lane's own:  (7 GH + 7 R) es
      the correction, 4 rounded quantities and the response's error, not propagated:           4 u (Sm + R Ym) + dh Ym
and D = 1.05 |g| (E_S sequential + E_S blocked) + 2 u |s|, the 1.05 for the terms of second order.  D is worst-case: for a
narrow filter at a low frequency (R in the hundreds) it is orders above what the blocked evaluation really does: on the two
filters of tests/test_biquad_spec.py, a 20 Hz high-pass and a 20 Hz low-pass of Q 10 at 48 kHz, the scan is 4.4e-10 and
2.1e-10 from the sequential evaluation -- not the 5e-12 of chunks whose state is carried one after the other, since a scan
applies powers of M over thousands of frames to partial states that are hundreds of times the signal -- and D is above 1.  Raw coefficients with poles on or outside the unit circle are data: their D
is huge or infinite, and they are held to the twin only.  Dseq = 1.05 |g| 2 E_S sequential + 2 u |s| (`bound="sequential"`)
is how far two sequential float64 evaluations of the cascade, in this form or another direct form with at most 9 rounded
quantities of at most Q a sample, may be from one another.

Where D says nothing the stage is held to what its number formats promise instead (tests/test_biquad_spec.py and
tests/test_biquad.py, on those two filters): a row is float32 in memory and "rounded once", so the float64 evaluation has to
stay below one float32 rounding of the row's peak, |blocked - s| <= 2^-24 max |s|, and the kernel within 2^-24 |s| + 2^-24
max |s| of s -- 2.7e-8 and 1.5e-9 on those rows.  That is a requirement the evaluation meets with a factor of 60 and of 7 to
spare, not a worst case derived from it: a sound worst case of that size does not exist for a scan in plain float64 there,
since the powers' own errors (6e-8 and 9e-7 against the exact powers, most of it the harmless part that all powers share)
times the partial states already exceed it.

The designers are the RBJ Audio EQ Cookbook's forms (sox's, torchaudio.functional.*_biquad's), float64, vectorised; the same
formulas on torch float64 tensors serve drawn parameters on the device (`Effects.draw`), so nothing is read back -- the
trigonometry is torch's, not the kernel's, as the decibels are in mix.py.

Everything but `biquad` needs no device.  `Corpus.crops(effects=)` and `Corpus.random_crops(effects=)` run the stage on the
waveform behind reverb= and mix= and in front of features=.
"""
import functools
import math
from fractions import Fraction

import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_device, _lengths_host, _lines, _planes, _Spec

# csrc/alac_biquad.h
CHUNK, THREADS, LEVELS, MAX_SECTIONS = 16, 256, 6, 8
TILE = CHUNK * THREADS
_LANES = 64
_U = 2.0 ** -53
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)
KINDS = ("lowpass", "highpass", "bandpass", "bandreject", "allpass", "peaking", "lowshelf", "highshelf")


# ---- the designers -------------------------------------------------------------------------------------------------------------
class _Np:
    sin, cos, sqrt, stack = np.sin, np.cos, np.sqrt, staticmethod(lambda parts: np.stack(parts, axis=-1))
    pow10 = staticmethod(lambda x: np.power(10.0, x))


def _torch_ops():
    import torch

    class _T:
        sin, cos, sqrt, stack = torch.sin, torch.cos, torch.sqrt, staticmethod(lambda parts: torch.stack(parts, dim=-1))
        pow10 = staticmethod(lambda x: torch.pow(10.0, x))
    return _T


def _design(m, kind, sample_rate, freq, q, gain_db):
    """The cookbook's formulas on float64 arrays of one shape (numpy or torch by `m`): [..., 5], a0 divided out"""
    w0 = (2.0 * math.pi) * freq / sample_rate
    cs, alpha = m.cos(w0), m.sin(w0) / (2.0 * q)
    one = cs * 0.0 + 1.0
    if kind == "lowpass":
        half = m.sin(w0 / 2.0)
        omc = 2.0 * half * half                     # 1 - cos w0 without the cancellation at low frequencies
        b, a = (omc / 2.0, omc, omc / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "highpass":
        b, a = ((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "bandpass":
        b, a = (alpha, 0.0 * cs, -alpha), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "bandreject":
        b, a = (one, -2.0 * cs, one), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "allpass":
        b, a = (1.0 - alpha, -2.0 * cs, 1.0 + alpha), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    else:
        A = m.pow10(gain_db / 40.0) * one
        if kind == "peaking":
            b, a = (1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A)
        else:
            k = 2.0 * m.sqrt(A) * alpha
            if kind == "lowshelf":
                b = (A * ((A + 1.0) - (A - 1.0) * cs + k), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * ((A + 1.0) - (A - 1.0) * cs - k))
                a = ((A + 1.0) + (A - 1.0) * cs + k, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - k)
            elif kind == "highshelf":
                b = (A * ((A + 1.0) + (A - 1.0) * cs + k), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * ((A + 1.0) + (A - 1.0) * cs - k))
                a = ((A + 1.0) - (A - 1.0) * cs + k, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - k)
            else:
                raise ValueError(f"kind must be one of {', '.join(KINDS)}, not {kind!r}")
    return m.stack([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def design(kind, sample_rate, freq, q=math.sqrt(0.5), gain_db=0.0):
    """The section (b0, b1, b2, a1, a2) of the cookbook's filter `kind` at `freq` Hz for signals at sample_rate: float64
    [..., 5] over the broadcast shape of the arguments (numbers or numpy arrays).  gain_db counts for the peaking filter and
    the shelves.  ValueError: a kind that is none of KINDS, freq outside 0 < f < sample_rate / 2, q <= 0, anything that is
    not finite."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {', '.join(KINDS)}, not {kind!r}")
    try:
        fs, f, qq, g = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (sample_rate, freq, q, gain_db)))
    except (TypeError, ValueError):
        raise ValueError("sample_rate, freq, q and gain_db must be numbers or arrays of one shape") from None
    if not (np.isfinite(fs).all() and np.isfinite(f).all() and np.isfinite(qq).all() and np.isfinite(g).all()):
        raise ValueError("sample_rate, freq, q and gain_db must be finite")
    if not ((f > 0).all() and (f < fs / 2).all()):
        raise ValueError("freq must be in 0 < freq < sample_rate / 2")
    if not (qq > 0).all():
        raise ValueError("q must be positive")
    return _design(_Np, kind, fs, f, qq, g)


def _designer(kind):
    def fn(sample_rate, freq, q=math.sqrt(0.5), gain_db=0.0):
        return design(kind, sample_rate, freq, q, gain_db)
    fn.__name__ = fn.__qualname__ = kind
    fn.__doc__ = f"design({kind!r}, sample_rate, freq, q, gain_db)"
    return fn


lowpass, highpass, bandpass, bandreject = (_designer(k) for k in KINDS[:4])
allpass, peaking, lowshelf, highshelf = (_designer(k) for k in KINDS[4:])


# ---- the policy ----------------------------------------------------------------------------------------------------------------
def _range(name, v, least=None):
    """v, a number or (lo, hi) with lo <= hi, as (lo, hi)"""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be a number or (lo, hi), not {v!r}")
        lo, hi = _f32_finite(f"{name}[0]", v[0]), _f32_finite(f"{name}[1]", v[1])
        if lo > hi:
            raise ValueError(f"{name} {v!r}: lo above hi")
    else:
        lo = hi = _f32_finite(name, v)
    if least is not None and not lo > least:
        raise ValueError(f"{name} must be above {least}, not {v!r}")
    return lo, hi


def _probability(p):
    p = _f32_finite("p", p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"p must be in 0 .. 1, not {p!r}")
    return p


class RandomBiquad(_Spec):
    """One section of an `Effects`: the cookbook's filter `kind` (one of KINDS) with freq in Hz, q and gain_db each a number
    or (lo, hi) with lo <= hi, drawn per crop -- freq uniformly on a log axis, the others linearly -- and p in 0 .. 1 the
    probability that a crop gets the section at all (else it is the identity).  Immutable; the three are kept as (lo, hi).
    ValueError: a kind that is none of KINDS, freq or q not positive, anything not finite."""

    __slots__ = ("kind", "freq", "q", "gain_db", "p")

    def __init__(self, kind, freq, q=0.7071, gain_db=0.0, p=1.0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {', '.join(KINDS)}, not {kind!r}")
        s = object.__setattr__
        s(self, "kind", kind)
        s(self, "freq", _range("freq", freq, least=0.0))
        s(self, "q", _range("q", q, least=0.0))
        s(self, "gain_db", _range("gain_db", gain_db))
        s(self, "p", _probability(p))


class Effects(_Spec):
    """The channel a crop goes through, for `Corpus.crops(effects=)` and `Corpus.random_crops(effects=)`: filters, a tuple of
    up to 8 `RandomBiquad`, in the order they run; gain (lo, hi), a linear factor drawn uniformly (Kaldi's volume perturbation
    is gain=(0.125, 2)), or gain_db (lo, hi), drawn uniformly in decibels -- not both; p in 0 .. 1: the probability that a
    crop gets any of it; clamp: the result is limited to -1 .. 1.  Immutable.  ValueError otherwise."""

    __slots__ = ("filters", "gain", "gain_db", "p", "clamp")

    def __init__(self, filters=(), gain=None, gain_db=None, p=1.0, clamp=False):
        if isinstance(filters, RandomBiquad):
            filters = (filters,)
        try:
            filters = tuple(filters)
        except TypeError:
            raise ValueError(f"filters must be a tuple of RandomBiquad, not {filters!r}") from None
        if len(filters) > MAX_SECTIONS or not all(isinstance(f, RandomBiquad) for f in filters):
            raise ValueError(f"filters must be at most {MAX_SECTIONS} RandomBiquad, not {filters!r}")
        if gain is not None and gain_db is not None:
            raise ValueError("gain and gain_db are exclusive")
        if not isinstance(clamp, (bool, np.bool_)):
            raise ValueError(f"clamp must be a bool, not {clamp!r}")
        s = object.__setattr__
        s(self, "filters", filters)
        s(self, "gain", None if gain is None else _range("gain", gain))
        s(self, "gain_db", None if gain_db is None else _range("gain_db", gain_db))
        s(self, "p", _probability(p))
        s(self, "clamp", bool(clamp))

    @classmethod
    def telephone(cls):
        """The telephone band: a fourth-order Butterworth high-pass at 300 Hz and low-pass at 3400 Hz, four fixed sections"""
        qs = (1.0 / (2.0 * math.cos(math.pi / 8.0)), 1.0 / (2.0 * math.cos(3.0 * math.pi / 8.0)))
        return cls(tuple(RandomBiquad(kind, f, q=q) for kind, f in (("highpass", 300.0), ("lowpass", 3400.0)) for q in qs))

    @property
    def sections(self):
        """S of the coefficients `draw` returns: the filters, one identity section without any"""
        return max(len(self.filters), 1)

    def check_rate(self, sample_rate):
        """ValueError for a filter whose frequency reaches the Nyquist frequency of sample_rate"""
        rate = _f32_finite("sample_rate", sample_rate, least=1.0)
        for f in self.filters:
            if not f.freq[1] < rate / 2.0:
                raise ValueError(f"a {f.kind} at up to {f.freq[1]} Hz on crops at {sample_rate} Hz: at or above Nyquist")
        return rate

    def draw(self, batch, sample_rate, generator=None, device=None):
        """The draws of `batch` crops at sample_rate: (coeffs float64 [B, S, 5], gain float64 [B]) on `device` (default: the
        generator's, else the current GPU).  One torch.rand of float64 [4 F + 2, B], whatever the arguments, so that a seeded
        generator reproduces them; its rows in order: per filter u for freq = exp(ln lo + (ln hi - ln lo) u), u for
        q = lo + (hi - lo) u, u for gain_db likewise, k (the crop gets the section where k < p); then u for the gain and k for
        the crop.  A section or a crop that loses its draw is the identity.  A filter whose three parameters are numbers is
        designed on the host, once per rate and device.  generator: a torch.Generator of the device or of the CPU (the draws
        are then made there and moved).  Nothing is read back.  ValueError: a freq at or above sample_rate / 2."""
        import torch

        from . import _frame_count

        rate = self.check_rate(sample_rate)
        B = _frame_count("batch", batch)
        if device is not None:
            here = torch.device(device)
        else:
            here = generator.device if generator is not None else torch.device("cuda", torch.cuda.current_device())
        dev = generator.device if generator is not None else here
        u = torch.rand((4 * len(self.filters) + 2, B), generator=generator, device=dev, dtype=torch.float64).to(here)
        ident = _fixed_section(None, 0.0, 0.0, 0.0, 0.0, str(here))
        ops = _torch_ops()
        rows = []
        for i, f in enumerate(self.filters):
            (f0, f1), (q0, q1), (g0, g1) = f.freq, f.q, f.gain_db
            if f0 == f1 and q0 == q1 and g0 == g1:
                sec = _fixed_section(f.kind, rate, f0, q0, g0, str(here)).expand(B, 5)
            else:
                freq = torch.exp(math.log(f0) + (math.log(f1) - math.log(f0)) * u[4 * i]).clamp(f0, f1)
                sec = _design(ops, f.kind, rate, freq, q0 + (q1 - q0) * u[4 * i + 1], g0 + (g1 - g0) * u[4 * i + 2])
            rows.append(sec if f.p >= 1.0 else torch.where((u[4 * i + 3] < f.p)[:, None], sec, ident))
        coeffs = torch.stack(rows, dim=1) if rows else ident.expand(B, 1, 5).clone()      # (never the cached tensor itself)
        if self.gain is not None:
            gain = self.gain[0] + (self.gain[1] - self.gain[0]) * u[-2]
        elif self.gain_db is not None:
            gain = torch.pow(10.0, (self.gain_db[0] + (self.gain_db[1] - self.gain_db[0]) * u[-2]) / 20.0)
        else:
            gain = torch.ones(B, dtype=torch.float64, device=here)
        if self.p < 1.0:
            keep = u[-1] < self.p
            coeffs, gain = torch.where(keep[:, None, None], coeffs, ident), torch.where(keep, gain, 1.0)
        return coeffs.contiguous(), gain


@functools.lru_cache(maxsize=256)
def _fixed_section(kind, sample_rate, freq, q, gain_db, device):
    """A section of fixed parameters (kind None: the identity) as a float64 tensor [5] on `device`, made once"""
    import torch

    sec = np.asarray(IDENTITY) if kind is None else design(kind, sample_rate, freq, q, gain_db)
    return torch.from_numpy(np.ascontiguousarray(sec, dtype=np.float64)).to(device)


# ---- the specification, its bound and the twin ---------------------------------------------------------------------------------
def _host_args(x, coeffs, lengths, gain):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 3 or x.shape[1] == 0:
        raise ValueError(f"x must be float32 [B, C, T], not {x.dtype} {x.shape}")
    B, C, T = x.shape
    try:
        q = np.asarray(coeffs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("coeffs must be numbers [B, S, 5] or [S, 5]") from None
    if q.ndim == 2:
        q = np.broadcast_to(q, (B,) + q.shape)
    if q.ndim != 3 or q.shape[0] != B or q.shape[2] != 5 or not 1 <= q.shape[1] <= MAX_SECTIONS:
        raise ValueError(f"coeffs must be [{B}, S, 5] or [S, 5] with 1 <= S <= {MAX_SECTIONS}, not {q.shape}")
    if gain is None:
        g = np.ones(B, dtype=np.float64)
    else:
        g = np.asarray(gain, dtype=np.float64)
        if g.shape != (B,):
            raise ValueError(f"gain must be {B} numbers, not {g.shape}")
    return x, np.ascontiguousarray(q), _lengths_host("lengths", lengths, B, T), g


def _live(q, g, clamp):
    """The rows that are not the identity"""
    return ~((q == np.asarray(IDENTITY)).all(axis=(1, 2)) & (g == 1.0)) | bool(clamp)


def _sequential(U, q):
    """u_S of U float64 [R, C, n] by q [R, S, 5], sample after sample; also the magnitudes (Um, Ym) [R, S] for the bound"""
    R, S = q.shape[:2]
    mags = np.zeros((2, R, S))
    with np.errstate(all="ignore"):
        for k in range(S):
            b0, b1, b2, a1, a2 = (q[:, k, i][:, None] for i in range(5))
            Y = np.empty_like(U)
            u1 = u2 = y1 = y2 = np.zeros(U.shape[:2])
            for n in range(U.shape[2]):
                u0 = U[:, :, n]
                y0 = b0 * u0 + b1 * u1 + b2 * u2 - a1 * y1 - a2 * y2
                Y[:, :, n] = y0
                u2, u1, y2, y1 = u1, u0, y1, y0
            mags[0, :, k] = np.abs(U).max(axis=(1, 2), initial=0.0)
            mags[1, :, k] = np.abs(Y).max(axis=(1, 2), initial=0.0)
            U = Y
    return U, mags


@functools.lru_cache(maxsize=4096)
def _table_error(a1, a2):
    """(dh, dP) of a section: how far `_tables` is from the exact homogeneous responses and powers, by integer arithmetic"""
    if not (math.isfinite(a1) and math.isfinite(a2)):
        return math.inf, math.inf
    h, P = _tables(np.array([[[1.0, 0.0, 0.0, a1, a2]]]))
    h, P = h[0, 0], P[0, 0]
    fa1, fa2 = Fraction(-a1), Fraction(-a2)
    k = max(fa1.denominator.bit_length(), fa2.denominator.bit_length()) - 1
    one = 1 << k
    A = ((int(fa1 * one), int(fa2 * one)), (one, 0))         # the transition matrix times 2^k

    def mul(X, Y):
        return tuple(tuple(X[i][0] * Y[0][j] + X[i][1] * Y[1][j] for j in range(2)) for i in range(2))

    def off(X, n, F):      # the row-sum norm of X / 2^(k n) - F
        d = [[abs(Fraction(X[i][j], 1 << (k * n)) - Fraction(float(F[i][j]))) for j in range(2)] for i in range(2)]
        return float(max(d[0][0] + d[0][1], d[1][0] + d[1][1]))

    dh, X = 0.0, A
    for j in range(CHUNK):       # X = A^(j + 1): its first row is (h1[j], h2[j])
        dh = max(dh, float(abs(Fraction(X[0][0], 1 << (k * (j + 1))) - Fraction(float(h[0, j])))
                           + abs(Fraction(X[0][1], 1 << (k * (j + 1))) - Fraction(float(h[1, j])))))
        if j + 1 < CHUNK:
            X = mul(X, A)
    dP, n = 0.0, CHUNK
    for i in range(LEVELS + 1):
        dP = max(dP, off(X, n, P[i]))
        X, n = mul(X, X), 2 * n
    return dh, dP


def _bound(q, g, mags, T, S_out):
    """(D, Dseq) [R] of the module docstring for rows of T frames: q [R, S, 5], g [R], mags from `_sequential`, S_out = max |s|
    [R]"""
    R, S = q.shape[:2]
    n = max(T, 1) + CHUNK
    Eseq, Eblk = np.zeros(R), np.zeros(R)
    with np.errstate(all="ignore"):
        for k in range(S):
            b0, b1, b2, a1, a2 = (q[:, k, i] for i in range(5))
            r = np.zeros((n + 2, R))                 # r[m + 2] is r[m]; r[-1] = r[-2] = 0
            r[2] = 1.0
            for m in range(1, n):
                r[m + 2] = -a1 * r[m + 1] - a2 * r[m]
            ar = np.abs(r)
            G = ar.sum(axis=0)
            Hs = np.maximum(ar[2:] + np.abs(a2) * ar[1:-1], ar[1:-1] + np.abs(a2) * ar[:-2])       # [n, R]
            Rm = np.maximum(Hs.max(axis=0), 1.0)
            pad = (-n) % CHUNK
            GH = np.concatenate([Hs, np.zeros((pad, R))]).reshape(-1, CHUNK, R).sum(axis=0).max(axis=0)
            err = np.array([_table_error(float(a1[i]), float(a2[i])) for i in range(R)]).reshape(R, 2)
            dh, dP = err[:, 0], err[:, 1]
            Bf, Af = np.abs(b0) + np.abs(b1) + np.abs(b2), np.abs(a1) + np.abs(a2)
            Um, Ym = mags[0, :, k], mags[1, :, k]
            Sm = (1.0 + Rm) * Ym
            Eseq = G * (Bf * Eseq + 9.0 * _U * (Bf * Um + Af * Ym))
            es = (4.0 * _U * (Rm + 1.0) + dP) * Sm
            Eblk = (G * (Bf * Eblk + _U * (5.0 * Bf * Um + 4.0 * (Bf * Um + Af * Sm))) + (7.0 * GH + 7.0 * Rm) * es
                    + 4.0 * _U * (Sm + Rm * Ym) + dh * Ym)
        Dseq = 1.05 * np.abs(g) * 2.0 * Eseq + 2.0 * _U * S_out
        D = 1.05 * np.abs(g) * (Eseq + Eblk) + 2.0 * _U * S_out
    return np.where(np.isnan(D), np.inf, D), np.where(np.isnan(Dseq), np.inf, Dseq)


def biquad_host(x, coeffs, lengths=None, gain=None, clamp=False, bound=False):
    """The specification in numpy: x float32 [B, C, T], coeffs [B, S, 5] or [S, 5] (as float64), lengths [B] integers
    (default T), gain [B] (default 1) to s float64 [B, C, T]: g u_S, unrounded, with `clamp` limited to -1 .. 1; x itself
    behind the lengths and in identity rows.  bound=True: returns (s, D), D float64 like s: how far a blocked float64
    evaluation may be from the sequential one (the module docstring); the kernel is within 2^-24 |s| + D of s.
    bound="sequential": returns (s, Dseq), how far two sequential float64 evaluations may be from one another."""
    x, q, v, g = _host_args(x, coeffs, lengths, gain)
    B, C, T = x.shape
    s = x.astype(np.float64)
    D = np.zeros(x.shape, dtype=np.float64)
    live = _live(q, g, clamp) & (v > 0)
    with np.errstate(all="ignore"):
        for length in np.unique(v[live]):          # the rows of one length together: the loop over the samples is Python's
            rows = np.nonzero(live & (v == length))[0]
            n = int(length)
            u, mags = _sequential(s[rows, :, :n], q[rows])
            y = g[rows, None, None] * u
            if bound:
                both = _bound(q[rows], g[rows], mags, n, np.abs(y).max(axis=(1, 2), initial=0.0))
                D[rows, :, :n] = both[1 if bound == "sequential" else 0][:, None, None]
            if clamp:
                y = np.where(np.isnan(y), y, np.minimum(np.maximum(y, -1.0), 1.0))
            s[rows, :, :n] = y
    return (s, D) if bound else s


def _tables(q):
    """The tables of every section, in the kernel's order: h float64 [R, S, 2, CHUNK] (h1, h2) and P [R, S, LEVELS + 1, 2, 2]"""
    R, S = q.shape[:2]
    a1, a2 = q[:, :, 3], q[:, :, 4]
    h = np.empty((R, S, 2, CHUNK))
    P = np.empty((R, S, LEVELS + 1, 2, 2))
    with np.errstate(all="ignore"):
        for i, (p1, p2) in enumerate(((1.0, 0.0), (0.0, 1.0))):
            p1, p2 = np.full((R, S), p1), np.full((R, S), p2)
            for j in range(CHUNK):
                p1, p2 = (-(a1 * p1)) - (a2 * p2), p1
                h[:, :, i, j] = p1
        P[:, :, 0, 0, 0], P[:, :, 0, 0, 1] = h[:, :, 0, CHUNK - 1], h[:, :, 1, CHUNK - 1]
        P[:, :, 0, 1, 0], P[:, :, 0, 1, 1] = h[:, :, 0, CHUNK - 2], h[:, :, 1, CHUNK - 2]
        for i in range(LEVELS):
            M = P[:, :, i]
            for r in range(2):
                for c in range(2):
                    P[:, :, i + 1, r, c] = (M[:, :, r, 0] * M[:, :, 0, c]) + (M[:, :, r, 1] * M[:, :, 1, c])
    return h, P


def _apply(P, t):
    """P t of the module docstring: P [..., 2, 2] (broadcast over the lanes), t = (t0, t1)"""
    return (P[..., 0, 0] * t[0]) + (P[..., 0, 1] * t[1]), (P[..., 1, 0] * t[0]) + (P[..., 1, 1] * t[1])


def _twin_rows(X, q, g):
    """The kernel's arithmetic on X float64 [R, n] (a row per (row, channel), its valid frames) with q [R, S, 5] and g [R]:
    float64 [R, n], g u_S"""
    R, n = X.shape
    S = q.shape[1]
    tiles = -(-n // TILE)
    U = np.zeros((R, tiles * TILE))
    U[:, :n] = X
    U = U.reshape(R, tiles, THREADS, CHUNK)
    out = np.empty_like(U)
    h, P = _tables(q)
    lane = np.arange(THREADS) % _LANES
    carry = np.zeros((S + 1, 2, R))                                  # the last two values of u_k in front of the tile
    with np.errstate(all="ignore"):
        for t in range(tiles):
            u = U[:, t].copy()                                           # [R, THREADS, CHUNK]
            # the input's history in front of every lane
            in0 = np.concatenate([carry[0, 0][:, None], u[:, :-1, CHUNK - 1]], axis=1)
            in1 = np.concatenate([carry[0, 1][:, None], u[:, :-1, CHUNK - 2]], axis=1)
            carry[0, 0], carry[0, 1] = u[:, -1, CHUNK - 1], u[:, -1, CHUNK - 2]
            for k in range(S):
                b0, b1, b2, a1, a2 = (q[:, k, i][:, None] for i in range(5))
                prev = np.concatenate([in1[:, :, None], in0[:, :, None], u], axis=2)          # u[j - 2] at index j
                w = ((b0[:, :, None] * prev[:, :, 2:]) + (b1[:, :, None] * prev[:, :, 1:-1])) + (b2[:, :, None] * prev[:, :, :-2])
                y1 = y2 = np.zeros((R, THREADS))
                y = np.empty_like(w)
                for j in range(CHUNK):
                    y0 = (w[:, :, j] - (a1 * y1)) - (a2 * y2)
                    y[:, :, j] = y0
                    y2, y1 = y1, y0
                s0, s1 = y[:, :, CHUNK - 1].copy(), y[:, :, CHUNK - 2].copy()
                for i in range(LEVELS):                                  # the scan within a wave
                    d = 1 << i
                    t0, t1 = np.roll(s0, d, axis=1), np.roll(s1, d, axis=1)
                    r0, r1 = _apply(P[:, k, i][:, None], (t0, t1))
                    on = lane >= d
                    s0, s1 = np.where(on, r0 + s0, s0), np.where(on, r1 + s1, s1)
                c0, c1 = carry[k + 1, 0].copy(), carry[k + 1, 1].copy()          # the state in front of every wave
                cw0, cw1 = np.empty((R, THREADS)), np.empty((R, THREADS))
                for wv in range(THREADS // _LANES):
                    cw0[:, wv * _LANES:(wv + 1) * _LANES], cw1[:, wv * _LANES:(wv + 1) * _LANES] = c0[:, None], c1[:, None]
                    r0, r1 = _apply(P[:, k, LEVELS], (c0, c1))
                    c0, c1 = r0 + s0[:, wv * _LANES + _LANES - 1], r1 + s1[:, wv * _LANES + _LANES - 1]
                carry[k + 1, 0], carry[k + 1, 1] = c0, c1
                q0, q1 = cw0, cw1
                for i in range(LEVELS):                                  # M^lane c_w
                    r0, r1 = _apply(P[:, k, i][:, None], (q0, q1))
                    on = ((lane >> i) & 1) == 1
                    q0, q1 = np.where(on, r0, q0), np.where(on, r1, q1)
                below = lane >= 1
                e0 = np.where(below, q0 + np.roll(s0, 1, axis=1), q0)
                e1 = np.where(below, q1 + np.roll(s1, 1, axis=1), q1)
                u = (y + (h[:, k, 0][:, None, :] * e0[:, :, None])) + (h[:, k, 1][:, None, :] * e1[:, :, None])
                in0, in1 = e0, e1
            out[:, t] = g[:, None, None] * u
    return out.reshape(R, tiles * TILE)[:, :n]


def biquad_host_twin(x, coeffs, lengths=None, gain=None, clamp=False):
    """The kernel's arithmetic in numpy, its blocking operation by operation with nothing fused (the module docstring): x
    float32 [B, C, T] to float32 [B, C, T].  The kernel equals it bit for bit."""
    x, q, v, g = _host_args(x, coeffs, lengths, gain)
    B, C, T = x.shape
    y = x.copy()
    live = _live(q, g, clamp) & (v > 0)
    with np.errstate(all="ignore"):
        for length in np.unique(v[live]):
            rows = np.nonzero(live & (v == length))[0]
            n = int(length)
            X = x[rows, :, :n].astype(np.float64).reshape(len(rows) * C, n)
            r = _twin_rows(X, np.repeat(q[rows], C, axis=0), np.repeat(g[rows], C)).astype(np.float32).reshape(len(rows), C, n)
            if clamp:
                r = np.where(np.isnan(r), r, np.minimum(np.maximum(r, np.float32(-1)), np.float32(1)))
            y[rows, :, :n] = r
    return y


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _f64_device(name, t, shape, device):
    """t (a tensor, a numpy array or a sequence of numbers) as a contiguous float64 tensor of `shape` on `device`"""
    import torch

    if isinstance(t, torch.Tensor):
        if tuple(t.shape) != shape or t.dtype == torch.bool or t.is_complex():
            raise ValueError(f"{name} must be numbers {list(shape)}, not {tuple(t.shape)} {t.dtype}")
        return t.to(device, torch.float64).contiguous()
    try:
        a = np.asarray(t, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be numbers {list(shape)}") from None
    if a.shape != shape:
        raise ValueError(f"{name} must be numbers {list(shape)}, not {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _biquad(ctx, x, coeffs, lengths, gain, clamp, out):
    """`biquad` behind its first check; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`)"""
    import torch

    stride = _planes("x", x)
    B, C, T = x.shape
    shape = tuple(coeffs.shape) if hasattr(coeffs, "shape") else np.shape(coeffs)
    if len(shape) not in (2, 3) or shape[-1] != 5 or not 1 <= shape[-2] <= MAX_SECTIONS or (len(shape) == 3 and shape[0] != B):
        raise ValueError(f"coeffs must be [{B}, S, 5] or [S, 5] with 1 <= S <= {MAX_SECTIONS}, not {tuple(shape)}")
    if not isinstance(clamp, (bool, np.bool_)):
        raise ValueError(f"clamp must be a bool, not {clamp!r}")
    if out is not None and out is not x and (
            not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
            or (x.numel() and (_lines(out) is None or _lines(out)[0] != stride))):
        raise ValueError("out must be x itself or a float32 tensor of x's shape, layout and device")
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    d_valid = _lengths_device("lengths", lengths, B, x.device)
    q = _f64_device("coeffs", coeffs, tuple(shape), x.device)
    if q.dim() == 2:
        q = q.expand(B, *q.shape).contiguous()
    g = None if gain is None else _f64_device("gain", gain, (B,), x.device)
    if out is None:
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        if x.numel():
            out.copy_(x)        # (what the kernel leaves untouched is x's)
    if x.numel() == 0:
        return out
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ctx().biquad_device(x, out, B, C, stride, T, d_valid, q, q.shape[1], g, bool(clamp), stream=stream)
    return out


def biquad(x, coeffs, lengths=None, gain=None, clamp=False, out=None):
    """A cascade of biquad sections and a gain per row on the GPU: x float32 [B, C, T] on the device, contiguous or the slice
    [..., :T] of a contiguous tensor (what lies behind the slice is neither read nor written).  coeffs: [B, S, 5] or [S, 5]
    for all rows, (b0, b1, b2, a1, a2) with a0 divided out, 1 <= S <= 8: host sequences and numpy arrays are uploaded, device
    tensors used as they are, as float64.  lengths: [B] integers, a sequence or a tensor (as `crops` returns them; -1 counts as
    0, more than T as T): the frames of a row that are filtered.  gain: [B] numbers (default 1).  clamp: the result is limited
    to -1 .. 1.  out: x itself (in place) or a tensor of x's shape and layout apart from it, of which the frames behind the
    lengths and the identity rows are left as they are; default: a new copy of x.  Returns out.  One launch, asynchronous on
    the current stream; ValueError before any device work."""
    ctx = _device_context("x", x, "[B, C, T]")
    return _biquad(ctx, x, coeffs, lengths, gain, clamp, out)
