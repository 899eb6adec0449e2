"""Per-channel energy normalisation (PCEN; Wang et al. 2017, `librosa.pcen`) behind the features in one launch
(alacgpu_pcen_device, csrc/alac_pcen.hip), the fourth kind of `normalize`'s `how` and the first that is a recurrence along time.
librosa is not at hand where this is built: the parity is with this written specification.

The data is float32 [B, ..., n] of energies (mel or constant-Q power, `log=None`); a line is the last dimension,
v = min(max(lengths[b], 0), n) its valid frames (n without lengths).  Pcen(b, gain, bias, power, eps, scale):

    s[t] = scale * x[t]
    M[0] = s[0];   M[t] = (1 - b) M[t-1] + b s[t]                       for 0 < t < v
    y[t] = (s[t] / (eps + M[t])^gain + bias)^power - bias^power          for t < v
    y[t] = 0                                                             for v <= t < n

M[0] = s[0] is the steady state of the smoother under a constant s[0], the initial condition `librosa.pcen` takes
(scipy.signal.lfilter with lfilter_zi * s[0]).  b = (sqrt(1 + 4 T^2) - 1) / (2 T^2) with T = time_constant * frame_rate,
librosa's; 0.024689453 for 0.4 s at 100 frames/s.  b, gain, bias and power are scalars or one value per line of a channel (per
mel bin: a trained front end at inference); line l of x [B, C, L, n] takes value l % L.  v = 0 -- a length of -1, a crop outside
the corpus, included -- is a line of zeros and reads nothing.  `pcen_host` is this in float64, sequentially, on the float32
input and the float32 values of the parameters (1 - b and bias^power in float64 from those).

The float32 arithmetic of the kernel, which `pcen_smoother_host_f32` (M) and `pcen_host_f32` (y) follow one IEEE operation at
a time, nothing contracted, bit for bit.  a = fl(1 - b), s[t] = fl(scale * x[t]).  The smoother is blocked: a team of P = 64
lanes (n <= 1024, a wave) or 256 (above, four waves) takes the line in passes of 4 P frames, lane i of the pass at p0 the frames
p0 + 4 i .. p0 + 4 i + 3:

  a lane   from m = 0, A = 1 over its frames t < v ascending: m = fl(fl(a m) + fl(b s[t])), A = fl(A a); at t = 0 instead
           m = s[0], A = 0.  m_k, A_k: m and A behind the lane's frame k.  Its map is (A, B) = (A_last, m_last): M behind its
           frames is A (M in front of them) + B.  A is a^k by repeated multiplication, never a power function.
  a wave   the inclusive scan of its 64 maps, for d = 1, 2, 4, 8, 16, 32 and every lane >= d at once, (A', B') the map of lane
           - d in front of the step: B = fl(fl(A B') + B), then A = fl(A A').
  a pass   c the carry into the pass (0 into the first); into wave 0 goes c_0 = c, into wave w + 1 c_{w+1} = fl(fl(A_w c_w) + B_w)
           with (A_w, B_w) the scanned map of lane 63 of wave w; the carry into the next pass is that behind the last wave.
           Into lane 0 of wave w goes C = c_w, into lane i > 0 C = fl(fl(A c_w) + B), (A, B) the scanned map of lane i - 1.
  a frame  M[t] = fl(fl(A_k C) + m_k).

The compression, per frame, with c = bias^power rounded once from float64:

    u = fl(eps + M);  g = exp2(fl(-gain * log2(u)));  w = fl(fl(s g) + bias);  y = fl(exp2(fl(power * log2(w))) - c)

log2 and exp2 are explicit polynomials (`_log2_f32`, `_exp2_f32`; alac_pcen_log2 and alac_pcen_exp2 of csrc/alac_pcen.h), not
the hardware's transcendental instructions: the whole result is specified bit for bit.
  log2 u   u = 2^e m, m in (sqrt(1/2), sqrt(2)] from the bits (a subnormal times 2^24 first); r = fl(fl(m - 1) / fl(m + 1)),
           z = fl(r r), q = L0 + z (L1 + z (L2 + z (L3 + z L4))) by Horner's rule, L_j = 2 / ((2 j + 1) ln 2);
           log2 u = fl(e + fl(r q)).  m - 1 is exact; m + 1, the division, z, q (its last step dominates: z <= 0.0295) and r q
           cost at most 6 u relative on |log2 m| <= 1/2, the series' next term 2e-9 of it, and the last addition u |log2 u|:
           |log2^ u - log2 u| <= u |log2 u| + DL,  DL = 4 u.
  exp2 p   k = rint(p), f = p - k exactly, |f| <= 1/2; q = 1 + f (E1 + f (... + f E7)), E_j = ln(2)^j / j!, by Horner's rule:
           every step's rounding is halved by the next multiplication, under 4 u in all, the coefficients' own under u, the
           series' next term 5e-9: a relative error of at most EE = 6 u; the scaling by 2^k in two steps is exact while the
           result is normal (one rounding of at most 2^-150 where it is subnormal).

The bound, with u = 2^-24 and everything not named exact.  Any evaluation of M[t] = sum_j c_tj s_j in which the path from
s_j to M[t] passes at most K_tj roundings is within sum_j gamma_K |c_tj| |s_j|.  Sequentially K = 3 (t - j) + 3: a's own rounding,
the product and the sum of every step, and s's and b s's.  Blocked, a^(t-j) is a product of t - j factors fl(a) however the
scan groups them (2 (t - j) roundings), and behind it come at most the 2 of b s, 6 of a lane's own steps, 12 of the wave's scan,
8 of the waves' carries, 2 of a pass's carry for every pass between j and t (at most t - j in all) and the 2 of the frame:
K <= 3 (t - j) + 32.  With Mabs the smoother of |s| (its own recurrence) and R[t] = a R[t-1] + 3 u Mabs[t], R[0] = 3 u |s[0]|,

    dM[t] = 1.01 (R[t] + 32 u Mabs[t])

bounds both orders against the exact M (1.01 for the terms of second order), so that the blocked and the sequential float32
smoothers are within 2 dM of one another: `pcen_smoother_host(..., bound=True)` returns dM.  Then, with U = eps + M, G = U^-gain,
W = s G + bias, Wp = W^power, all exact, and x^+ = exp(x) - 1:

    dU  = dM + u (|U| + dM)                               U_lo = U - dU > 0
    dl1 = dU / (U_lo ln 2) + u |log2 U| (1 + u) + DL      the argument, the last addition, the polynomial
    dp1 = gain dl1 + u (gain |log2 U| + gain dl1)
    rg  = (ln 2 dp1)^+ (1 + EE) + EE                      g's relative error
    dW  = |s G| ((1 + rg) (1 + u)^2 - 1) + u (|W| + |s G| (rg + 3 u))    s's rounding, the product, the sum;   W_lo = W - dW > 0
    dl2 = dW / (W_lo ln 2) + u |log2 W| (1 + u) + DL
    dp2 = power dl2 + u (power |log2 W| + power dl2)
    rw  = (ln 2 dp2)^+ (1 + EE) + EE
    dY  = Wp rw + u bias^power + u (|y| + Wp rw + u bias^power) + 2^-149

`pcen_host(..., bound=True)` returns dY: relative to Wp, not to y, because the final subtraction cancels (x = 0 throughout gives
bias^power - c, one rounding of c from zero).  The magnification is |gain log2 U| and |power log2 W|: an energy of 2^40 costs
40 u ln 2 in g before anything else is rounded.  Where U_lo or W_lo is not above zero, or anything is not finite, dY is inf or
NaN: no bound is claimed there.

What is not finite follows IEEE arithmetic and is never hidden.  A NaN or an infinity at t0 < v reaches M at the frames
t0 .. v - 1 of its own line and no other line and no earlier frame: a lane's own steps go forward, and a carry comes only from
the lanes and passes in front.  A NaN makes y a NaN at all of them; an infinity makes y a NaN at t0 (inf * inf^-gain = inf * 0)
and bias^power - c behind it, where s / inf^gain is 0 again.  One at or behind v is never read.  A negative energy gives whatever log2 of a negative u
or w gives: NaN.  (An infinity inside stays an infinity in the sequential order; blocked, where a^k has underflowed to zero in
a scanned map, 0 * inf makes it a NaN: not finite either way.)

`Pcen`, `pcen_host`, `pcen_smoother_host`, `pcen_smoother_host_f32` and `pcen_host_f32` need no device; `pcen` is the call on
device tensors, and normalize.normalize takes a `Pcen` by handing it on.
"""
import math

import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_host, _Spec

_U = 2.0 ** -24
CHUNK = 4                         # ALAC_PCEN_CHUNK of csrc/alac_pcen.h
WAVE_MAX = 1024                   # ALAC_PCEN_WAVE_MAX: up to here a team is 64 lanes, above LINE_THREADS
LINE_THREADS = 256                # ALAC_PCEN_LINE_THREADS
_DL, _EE = 4 * _U, 6 * _U         # the polynomials' errors (the module docstring)
_LOG2_COEF = (0.3205988980, 0.4121985831, 0.5770780164, 0.9617966939, 2.8853900818)          # L4 .. L0, as alac_pcen.h writes them
_EXP2_COEF = (1.5252734e-05, 1.5403530e-04, 1.3333558e-03, 9.6181291e-03, 5.5504109e-02, 2.4022651e-01, 6.9314718e-01)     # E7 .. E1
_KINDS = ("b", "gain", "bias", "power")
_TABLES = {}                      # (spec, device index) -> the float32 device tensor [5, L] of a per-bin spec


def smoothing_coefficient(time_constant, frame_rate):
    """b = (sqrt(1 + 4 T^2) - 1) / (2 T^2), T = time_constant * frame_rate: librosa.pcen's"""
    T = float(time_constant) * float(frame_rate)
    if not math.isfinite(T) or T <= 0.0:
        raise ValueError(f"time_constant * frame_rate must be finite and above 0, not {T!r}")
    return (math.sqrt(1.0 + 4.0 * T * T) - 1.0) / (2.0 * T * T)


class Pcen(_Spec):
    """Per-channel energy normalisation of energies: (scale x / (eps + M)^gain + bias)^power - bias^power, M the first-order
    smoothing of scale x along a line with coefficient b from M[0] = scale x[0].  Exactly one of b and frame_rate is given:
    with frame_rate (frames per second) b follows from time_constant (seconds) as in librosa.  b, gain, bias and power are
    each a number or a sequence with one value per line of a channel (per mel bin); the sequences have one length, `lines`.
    The defaults are librosa's but scale: librosa's default 2^31 is for a waveform in -1 .. 1.  Immutable.  ValueError unless
    0 < b <= 1, gain >= 0, bias >= 0, power > 0, eps > 0 and scale > 0 in float32, all finite."""

    __slots__ = ("b", "gain", "bias", "power", "eps", "scale")

    def __init__(self, b=None, *, time_constant=0.4, frame_rate=None, gain=0.98, bias=2.0, power=0.5, eps=1e-6, scale=1.0):
        s = object.__setattr__
        if (b is None) == (frame_rate is None):
            raise ValueError("exactly one of b and frame_rate is given")
        if b is None:
            b = smoothing_coefficient(_f32_finite("time_constant", time_constant), _f32_finite("frame_rate", frame_rate))
        lines = None
        for name, v in zip(_KINDS, (b, gain, bias, power)):
            if isinstance(v, (list, tuple, np.ndarray)):
                if np.ndim(v) != 1 or len(v) == 0:
                    raise ValueError(f"{name} must be a number or a sequence of numbers with one value per line")
                v = tuple(_f32_finite(name, a.item() if isinstance(a, np.generic) else a) for a in v)
                if lines is not None and len(v) != lines:
                    raise ValueError(f"{name} has {len(v)} values, another parameter {lines}")
                lines = len(v)
                each = v
            else:
                v = _f32_finite(name, v)
                each = (v,)
            for a in each:
                a32 = float(np.float32(a))
                if ((name == "b" and not 0.0 < a32 <= 1.0) or (name == "power" and not a32 > 0.0)
                        or (name in ("gain", "bias") and not a32 >= 0.0)):
                    raise ValueError(f"{name} must be {dict(b='in (0, 1]', power='above 0').get(name, 'at least 0')} in float32, not {a!r}")
            s(self, name, v)
        for name, v in (("eps", eps), ("scale", scale)):
            v = _f32_finite(name, v)
            if not float(np.float32(v)) > 0.0:
                raise ValueError(f"{name} must be above 0 in float32, not {v!r}")
            s(self, name, v)

    @classmethod
    def like(cls, spec, **kw):
        """The Pcen whose frame rate is that of `spec`, a features.LogMel, a fbank.KaldiFbank, a cqt.ConstantQ or a stft.Spectrogram:
        sample_rate / hop_length.  kw: the other arguments of `Pcen` (time_constant among them)."""
        from .cqt import ConstantQ
        from .fbank import KaldiFbank
        from .features import LogMel
        from .stft import Spectrogram

        if not isinstance(spec, (LogMel, KaldiFbank, ConstantQ, Spectrogram)):
            raise ValueError(f"spec must be a features.LogMel, a fbank.KaldiFbank or a cqt.ConstantQ or a stft.Spectrogram, not {spec!r}")
        if "b" in kw or "frame_rate" in kw:
            raise ValueError("Pcen.like takes the frame rate from spec: neither b nor frame_rate")
        return cls(frame_rate=spec.sample_rate / spec.hop_length, **kw)

    @property
    def lines(self):
        """The length of the per-line sequences, or None where every parameter is a number"""
        for name in _KINDS:
            if isinstance(getattr(self, name), tuple):
                return len(getattr(self, name))
        return None

    def table(self):
        """float32 [5, lines or 1]: b, gain, bias, power and bias^power -- from float64 on the float32 values, rounded once --
        per line of a channel: alacgpu_pcen_device's d_table, and the scalars of a spec without sequences"""
        L = self.lines or 1
        t = np.empty((5, L), dtype=np.float32)
        for k, name in enumerate(_KINDS):
            t[k] = np.asarray(getattr(self, name), dtype=np.float64)
        t[4] = t[2].astype(np.float64) ** t[3].astype(np.float64)
        return t


def _host_args(x, how, lengths):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 2:
        raise ValueError(f"x must be float32 [B, ..., n], not {x.dtype} {x.shape}")
    if not isinstance(how, Pcen):
        raise ValueError(f"how must be a Pcen, not {how!r}")
    if how.lines is not None and (x.ndim != 4 or x.shape[2] != how.lines):
        raise ValueError(f"a Pcen with {how.lines} values per parameter needs x [B, C, {how.lines}, n], not {x.shape}")
    return x, _lengths_host("lengths", lengths, x.shape[0], x.shape[-1])


def _per_line(how, lines, dtype):
    """b, gain, bias, power, bias^power as [lines, 1] arrays of dtype holding the float32 values: line l takes column l % L"""
    t = how.table()
    at = np.arange(lines) % t.shape[1]
    if dtype == np.float64:           # the specification's bias^power is the exact one
        t = t.astype(np.float64)
        t[4] = t[2] ** t[3]
    return [t[k][at][:, None].astype(dtype) for k in range(5)]


def pcen_smoother_host(x, how, lengths=None, bound=False):
    """M of the specification: x float32 [B, ..., n] to float64 of that shape, sequentially, zeros at and behind v.
    bound=True: returns (M, dM), how far a float32 smoother, blocked or sequential, may be from M (the module docstring)."""
    x, lens = _host_args(x, how, lengths)
    shape = x.shape
    n = shape[-1]
    M = np.zeros(shape, dtype=np.float64)
    dM = np.zeros(shape, dtype=np.float64) if bound else None
    scale = float(np.float32(how.scale))
    with np.errstate(all="ignore"):
        for r in range(shape[0]):
            v = int(lens[r])
            if v == 0:
                continue
            S = scale * x[r].reshape(-1, n)[:, :v].astype(np.float64)
            b = _per_line(how, S.shape[0], np.float64)[0][:, 0]
            a = 1.0 - b
            out, err = np.empty_like(S), np.empty_like(S)
            m = S[:, 0].copy()
            mabs = np.abs(m)
            R = 3 * _U * mabs
            out[:, 0], err[:, 0] = m, R + 32 * _U * mabs
            for t in range(1, v):
                m = a * m + b * S[:, t]
                out[:, t] = m
                if bound:
                    mabs = a * mabs + b * np.abs(S[:, t])
                    R = a * R + 3 * _U * mabs
                    err[:, t] = R + 32 * _U * mabs
            M[r].reshape(-1, n)[:, :v] = out
            if bound:
                dM[r].reshape(-1, n)[:, :v] = 1.01 * err
    return (M, dM) if bound else M


def pcen_host(x, how, lengths=None, bound=False):
    """The specification in numpy: x float32 [B, ..., n] to float64 of that shape -- float64 arithmetic on the float32 input
    and the float32 values of `how`'s parameters.  lengths: [B] integers (below 0 counts as 0, above n as n); default: whole
    lines.  bound=True: returns (y, dY), dY float64 like y: how far the kernel's float32 arithmetic may be from y (the module
    docstring's chain; inf or NaN where it claims nothing)."""
    x, lens = _host_args(x, how, lengths)
    shape = x.shape
    n = shape[-1]
    M, dM = pcen_smoother_host(x, how, lengths, bound=True) if bound else (pcen_smoother_host(x, how, lengths), None)
    y = np.zeros(shape, dtype=np.float64)
    dY = np.zeros(shape, dtype=np.float64) if bound else None
    scale, eps = float(np.float32(how.scale)), float(np.float32(how.eps))
    ln2 = math.log(2.0)
    with np.errstate(all="ignore"):
        for r in range(shape[0]):
            v = int(lens[r])
            if v == 0:
                continue
            S = scale * x[r].reshape(-1, n)[:, :v].astype(np.float64)
            _, gain, bias, power, c = _per_line(how, S.shape[0], np.float64)
            U = eps + M[r].reshape(-1, n)[:, :v]
            G = U ** -gain
            W = S * G + bias
            Wp = W ** power
            out = Wp - c
            y[r].reshape(-1, n)[:, :v] = out
            if not bound:
                continue
            E = dM[r].reshape(-1, n)[:, :v]
            dU = E + _U * (np.abs(U) + E)
            U_lo = U - dU
            l1 = np.abs(np.log2(U))
            dl1 = dU / (U_lo * ln2) + _U * l1 * (1 + _U) + _DL
            dp1 = gain * dl1 + _U * (gain * l1 + gain * dl1)
            rg = np.expm1(ln2 * dp1) * (1 + _EE) + _EE
            sg = np.abs(S * G)
            dW = sg * ((1 + rg) * (1 + _U) ** 2 - 1) + _U * (np.abs(W) + sg * (rg + 3 * _U))
            W_lo = W - dW
            l2 = np.abs(np.log2(W))
            dl2 = dW / (W_lo * ln2) + _U * l2 * (1 + _U) + _DL
            dp2 = power * dl2 + _U * (power * l2 + power * dl2)
            rw = np.expm1(ln2 * dp2) * (1 + _EE) + _EE
            first = Wp * rw + _U * c
            err = first + _U * (np.abs(out) + first) + 2.0 ** -149
            err = np.where((U_lo > 0) & (W_lo > 0), err, np.inf)
            dY[r].reshape(-1, n)[:, :v] = np.where(np.isfinite(out), err, np.nan)
    return (y, dY) if bound else y


# ---- the kernel's arithmetic --------------------------------------------------------------------------------------------------
def _log2_f32(u):
    """alac_pcen_log2 of csrc/alac_pcen.h on a float32 array, operation by operation"""
    f32 = np.float32
    u = np.asarray(u, dtype=f32)
    with np.errstate(all="ignore"):
        ok = (u > 0) & (u != f32(np.inf))
        w = np.where(ok, u, f32(1.0))
        sub = w < f32(1.17549435e-38)
        w = np.where(sub, (w * f32(16777216.0)).astype(f32), w)
        e = np.where(sub, f32(-24.0), f32(0.0)).astype(f32)
        bits = np.ascontiguousarray(w).view(np.uint32)
        mant = bits & np.uint32(0x7FFFFF)
        up = mant > np.uint32(0x3504F3)
        m = (mant | np.where(up, np.uint32(0x3F000000), np.uint32(0x3F800000))).astype(np.uint32).view(f32)
        e = (e + ((bits >> np.uint32(23)).astype(np.int32) - 127 + up.astype(np.int32)).astype(f32)).astype(f32)
        r = ((m - f32(1.0)).astype(f32) / (m + f32(1.0)).astype(f32)).astype(f32)
        z = (r * r).astype(f32)
        q = np.full(u.shape, f32(_LOG2_COEF[0]), dtype=f32)
        for c in _LOG2_COEF[1:]:
            q = ((q * z).astype(f32) + f32(c)).astype(f32)
        res = (e + (r * q).astype(f32)).astype(f32)
        res = np.where(u == f32(np.inf), f32(np.inf), res)
        res = np.where(u == 0, f32(-np.inf), res)
        return np.where((u < 0) | np.isnan(u), f32(np.nan), res).astype(f32)


def _exp2_f32(p):
    """alac_pcen_exp2 of csrc/alac_pcen.h on a float32 array, operation by operation"""
    f32 = np.float32
    p = np.asarray(p, dtype=f32)
    with np.errstate(all="ignore"):
        ok = (p < f32(128.0)) & (p >= f32(-150.0))
        w = np.where(ok, p, f32(0.0))
        k = np.rint(w).astype(f32)
        f = (w - k).astype(f32)
        q = np.full(p.shape, f32(_EXP2_COEF[0]), dtype=f32)
        for c in _EXP2_COEF[1:] + (1.0,):
            q = ((q * f).astype(f32) + f32(c)).astype(f32)
        ki = k.astype(np.int32)
        k1 = ki >> 1
        k2 = ki - k1
        res = ((q * np.ldexp(f32(1.0), k1).astype(f32)).astype(f32) * np.ldexp(f32(1.0), k2).astype(f32)).astype(f32)
        res = np.where(p < f32(-150.0), f32(0.0), res)
        res = np.where(p >= f32(128.0), f32(np.inf), res)
        return np.where(np.isnan(p), f32(np.nan), res).astype(f32)


def _smoother_f32(S, a, b, n):
    """The blocked smoother of the lines S [lines, v] float32 (already scaled) of a tensor whose lines have n frames; a, b
    [lines, 1] float32.  Returns M [lines, v] float32."""
    f32 = np.float32
    lines, v = S.shape
    P = 64 if n <= WAVE_MAX else LINE_THREADS
    waves, span = P // 64, P * CHUNK
    M = np.zeros((lines, v), dtype=f32)
    carry = np.zeros((lines, 1), dtype=f32)
    for p0 in range(0, v, span):
        seg = np.zeros((lines, span), dtype=f32)
        k = min(span, v - p0)
        seg[:, :k] = S[:, p0:p0 + k]
        seg = seg.reshape(lines, P, CHUNK)
        t = p0 + np.arange(span).reshape(P, CHUNK)
        m = np.zeros((lines, P), dtype=f32)
        A = np.ones((lines, P), dtype=f32)
        mk, Ak = [], []
        for c in range(CHUNK):
            s = seg[:, :, c]
            step_m = ((a * m).astype(f32) + (b * s).astype(f32)).astype(f32)
            step_A = (A * a).astype(f32)
            first, on = (t[:, c] == 0)[None, :], (t[:, c] < v)[None, :]
            m = np.where(first, s, np.where(on, step_m, m))
            A = np.where(first, f32(0.0), np.where(on, step_A, A))
            mk.append(m)
            Ak.append(A)
        IA, IB = A.reshape(lines, waves, 64).copy(), m.reshape(lines, waves, 64).copy()
        d = 1
        while d < 64:
            pa, pb = IA[:, :, :-d].copy(), IB[:, :, :-d].copy()
            IB[:, :, d:] = ((IA[:, :, d:] * pb).astype(f32) + IB[:, :, d:]).astype(f32)
            IA[:, :, d:] = (IA[:, :, d:] * pa).astype(f32)
            d *= 2
        C = np.empty((lines, waves, 64), dtype=f32)
        c_w = carry
        for w in range(waves):
            C[:, w, :1] = c_w
            C[:, w, 1:] = ((IA[:, w, :-1] * c_w).astype(f32) + IB[:, w, :-1]).astype(f32)
            c_w = ((IA[:, w, 63:] * c_w).astype(f32) + IB[:, w, 63:]).astype(f32)
        carry = c_w
        C = C.reshape(lines, P)
        out = np.stack([((Ak[c] * C).astype(f32) + mk[c]).astype(f32) for c in range(CHUNK)], axis=2).reshape(lines, span)
        M[:, p0:p0 + k] = out[:, :k]
    return M


def _twin(x, how, lengths, smoother_only):
    x, lens = _host_args(x, how, lengths)
    f32 = np.float32
    shape = x.shape
    n = shape[-1]
    y = np.zeros(shape, dtype=f32)
    scale, eps = f32(how.scale), f32(how.eps)
    with np.errstate(all="ignore"):
        for r in range(shape[0]):
            v = int(lens[r])
            if v == 0:
                continue
            S = (scale * x[r].reshape(-1, n)[:, :v]).astype(f32)
            b, gain, bias, power, c = _per_line(how, S.shape[0], f32)
            M = _smoother_f32(S, (f32(1.0) - b).astype(f32), b, n)
            if not smoother_only:
                u = (eps + M).astype(f32)
                g = _exp2_f32(((-gain) * _log2_f32(u)).astype(f32))
                w = ((S * g).astype(f32) + bias).astype(f32)
                M = (_exp2_f32((power * _log2_f32(w)).astype(f32)) - c).astype(f32)
            y[r].reshape(-1, n)[:, :v] = M
    return y


def pcen_smoother_host_f32(x, how, lengths=None):
    """The kernel's M (stage 1) in numpy, bit for bit: x float32 [B, ..., n] to float32 of that shape, the blocked scan of the
    module docstring one float32 operation at a time; zeros at and behind v"""
    return _twin(x, how, lengths, True)


def pcen_host_f32(x, how, lengths=None):
    """The kernel's arithmetic in numpy, bit for bit: x float32 [B, ..., n] to float32 of that shape, the blocked smoother and
    the compression with the two polynomials, one float32 operation at a time"""
    return _twin(x, how, lengths, False)


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _table_device(how, device):
    """The float32 device tensor [5, how.lines] of a per-bin spec: uploaded once per (spec, device) and kept"""
    import torch

    key = (how, device.index if device.index is not None else torch.cuda.current_device())
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) >= 64:
            _TABLES.pop(next(iter(_TABLES)))
        t = _TABLES[key] = torch.from_numpy(how.table()).to(device)
    return t


def _launch(gpu, x, out, rows, lines_per_row, S, n, d_valid, how, stream, stage=0):
    """The one library call of a Pcen: the scalars, or the kept table of a per-bin spec"""
    if how.lines is None:
        b, gain, bias, power, c = (float(a) for a in how.table()[:, 0])
        gpu.pcen_device(x, out, rows, lines_per_row, S, n, d_valid, b, gain, bias, power, c, how.eps, how.scale, stage=stage, stream=stream)
    else:
        gpu.pcen_device(x, out, rows, lines_per_row, S, n, d_valid, 0.0, 0.0, 0.0, 0.0, 0.0, how.eps, how.scale,
                        d_table=_table_device(how, x.device), lines_per_param=how.lines, stage=stage, stream=stream)


def pcen(x, how, lengths=None, out=None):
    """Per-channel energy normalisation on the GPU: x float32 [B, ..., n] of energies on the device, contiguous or the slice
    [..., :n] of a contiguous tensor; what lies behind the slice is neither read nor written.  how: a `Pcen`; one with per-bin
    sequences needs x [B, C, L, n] with L their length.  lengths: [B] integers, a sequence or a tensor (as `crops` returns
    them; -1 counts as 0, more than n as n); default: whole lines; zeros behind them.  out: x itself (in place) or a tensor of
    x's shape and layout; default: a new one of x's layout.  Returns out.  One launch, asynchronous on the current stream;
    ValueError before any device work.  normalize.normalize(x, how, lengths, out) is the same call."""
    from .normalize import _normalize

    ctx = _device_context("x", x, "[B, ..., n]")
    if not isinstance(how, Pcen):
        raise ValueError(f"how must be a Pcen, not {how!r}")
    return _normalize(ctx, x, how, lengths, out)
