"""Fundamental frequency behind the crops: the YIN estimator (de Cheveigne and Kawahara, JASA 111 (4), 2002, steps 1 to 5 --
what `librosa.yin` computes), one launch (alacgpu_yin_device, csrc/alac_yin.hip).  Neither librosa nor torchaudio is at hand
where this is built: the parity is with this written specification, not with foreign fixtures.

Yin(sample_rate, win_length = W, hop_length, fmin, fmax, threshold, center, align_length):

    tau_min = floor(sample_rate / fmax),  tau_max = ceil(sample_rate / fmin),  span = W + tau_max

A row is x float32 with v = min(max(lengths[b], 0), T) valid samples (T without lengths); samples outside [0, v) read as
zero, nothing is reflected.  center=True: v // hop + 1 frames (`LogMel`'s count), frame t centred on c_t = t hop; center=False:
1 + (v - align_length) // hop frames, none for v < align_length (Kaldi's snip_edges count), c_t = t hop + align_length // 2.
The frame's first sample is s = c_t - span // 2.  Per frame:

    1.  d[tau]  = sum_{j < W} (x[s + j] - x[s + j + tau])^2,  tau = 0 .. tau_max: the direct sum of non-negative terms, never
                  energies minus an autocorrelation, which cancels
    2.  c[tau]  = d[1] + .. + d[tau];  d'[0] = 1,  d'[tau] = d[tau] tau / c[tau], 1 where c[tau] == 0.  c[tau_max] == 0
                  (silence, a constant): f0 = 0, ap = 1, and the frame is done
    3.  tau: the first of tau_min .. tau_max - 1 with d'[tau] < threshold, then forward while tau + 1 <= tau_max - 1 and
                  d'[tau + 1] < d'[tau]; without one below the threshold the first argmin of d' over that range
    4.  a, b, c = d'[tau - 1], d'[tau], d'[tau + 1]:  shift = 0.5 (a - c) / (a - 2 b + c) when b <= a, b <= c and the
                  denominator is positive, else 0
    5.  f0 = sample_rate / (tau + shift),  ap = b

The output is float32 [B, C, 2, T'] (T' = frames(T)): line 0 is f0 in Hz, always the best candidate; line 1 is ap, the
aperiodicity, and the frame is voiced exactly when ap < threshold (`Yin.voiced`).  Frames at and behind the row's frame count
are zero in both lines.

A NaN sample: every compare is IEEE's, and in the argmin a NaN counts as +infinity.  d[tau] is NaN for every lag whose sum
reaches the sample, c and d' from the first such lag on; a NaN d' is not below the threshold, ends a descent and is never the
argmin unless every candidate is one (then tau = tau_min), steps 4's compares fail (shift 0), and ap is NaN -- unvoiced -- when
the chosen lag's d' is.  Frames whose span does not hold the sample are what they are without it.

`yin_host` is the above in float64 on the float32 input (threshold and sample_rate as their float32 values).
`yin_host_f32` is the kernel, operation by operation, and equals it bit for bit:

    1.  per lag, acc = 0, then for j = 0 .. W - 1 in order: e = fl(x[s + j] - x[s + j + tau]), acc = fma(e, e, acc)
    2.  the lags 1 .. tau_max in chunks of 64 (zeros behind tau_max): within a chunk the inclusive scan v[l] = fl(v[l] +
        v[l - h]) for l >= h, h = 1, 2, 4, 8, 16, 32 (all l at once per h); c = fl(carry + v), carry = the chunk's last c,
        0 in front of the first;  d' = fl(fl(d float(tau)) / c), the division correctly rounded
    4.  n = fl(a - c),  q = fl(fl(a - 2 b) + c),  shift = fl((0.5 n) / q)
    5.  f0 = fl(float(sample_rate) / fl(float(tau) + shift))

The order is per frame and per lag: which frames share a workgroup (`tile_frames`) does not change a bit.

How far any correct float32 evaluation is from the specification, with u = 2^-24 and gamma_k = k u / (1 - k u): a term of d
is e^2 with e rounded once, and joins W accumulations at most, and every term is non-negative, so d is within gamma_{W + 2} of
the exact sum relatively, whatever the order.  c[tau] adds at most tau_max such values, again non-negative: within
gamma_{W + 2 + tau_max}.  d' takes a product and a division more: relatively within

    E = gamma_{2 (W + 2) + tau_max + 2}                                  (`dprime_bound`; 7.7e-5 at the defaults)

Every data-dependent choice of a frame -- the threshold compares, the descent's compares, the argmin, the two compares of step
4 -- compares two values p, q known within E (the threshold exactly), so it cannot flip while |p - q| / (|p| + |q|) > E
(|p - threshold| / |p| for the threshold).  `yin_host(..., margin=True)` returns the smallest of those quotients per frame: a
frame whose margin exceeds E chooses the same tau, and the same branch of step 4, in any correct float32 evaluation.  Then ap
is within E ap, and with kappa = (a + 2 b + c) / (a - 2 b + c) (0 where shift is 0), eta = (E + 2 u) kappa < 1,

    |shift' - shift| <= S = (E + 2 u) kappa / (1 - eta) + u          (|shift| <= 1/2: |a - c| <= a - 2 b + c for b <= a, c)
    |f0' - f0| / f0  <= S / (tau - 1/2) + 3 u                          (`f0_bound`)

`Yin`, `yin_host`, `yin_host_f32`, `dprime_bound`, `f0_bound`, `tile_frames` and `hz_to_cents` need no device; `yin` is the
call on device tensors.
"""
import math

import numpy as np

from ._stageargs import _device_context, _f32_finite, _fma32, _lengths_device, _lengths_host, _planes, _span, _Spec

_U = 2.0 ** -24
MIN_WIN, MAX_WIN, MAX_LAG = 64, 2048, 2048     # ALAC_YIN_MIN_WIN, ALAC_YIN_MAX_WIN, ALAC_YIN_MAX_LAG of csrc/alac_yin.h
TILE_MAX, LDS_FLOATS = 8, 8192                 # ALAC_YIN_TILE_MAX, ALAC_YIN_LDS_FLOATS


def _gamma(k):
    return k * _U / (1.0 - k * _U)


def _int(name, v, least, most=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < least or (most is not None and int(v) > most):
        raise ValueError(f"{name} must be an integer of at least {least}{'' if most is None else f' and at most {most}'}, not {v!r}")
    return int(v)


class Yin(_Spec):
    """An immutable description of the YIN estimator (see the module).  ValueError: sample_rate no positive integer below
    2^31, win_length no multiple of 64 in 64 .. 2048, tau_min < 2, tau_max <= tau_min + 1, tau_max > 2048, threshold outside
    (0, 1], hop_length < 1, center=False without align_length >= 1, a number that is not finite in float32."""

    __slots__ = ("sample_rate", "win_length", "hop_length", "fmin", "fmax", "threshold", "center", "align_length", "tau_min", "tau_max")

    def __init__(self, sample_rate, win_length=512, hop_length=160, fmin=60.0, fmax=400.0, threshold=0.1, center=True, align_length=None):
        s = object.__setattr__
        s(self, "sample_rate", _int("sample_rate", sample_rate, 1, (1 << 31) - 1))
        W = _int("win_length", win_length, MIN_WIN, MAX_WIN)
        if W % 64:
            raise ValueError(f"win_length must be a multiple of 64 in {MIN_WIN} .. {MAX_WIN}, not {win_length!r}")
        s(self, "win_length", W)
        s(self, "hop_length", _int("hop_length", hop_length, 1, (1 << 31) - 1))
        fmin, fmax = _f32_finite("fmin", fmin), _f32_finite("fmax", fmax)
        if not (fmin > 0.0 and fmax > 0.0):
            raise ValueError(f"fmin and fmax must be positive, not {fmin!r} and {fmax!r}")
        s(self, "fmin", fmin)
        s(self, "fmax", fmax)
        tau_min, tau_max = math.floor(self.sample_rate / fmax), math.ceil(self.sample_rate / fmin)
        if tau_min < 2:
            raise ValueError(f"fmax {fmax!r} at {self.sample_rate} Hz: the shortest lag {tau_min} is below 2")
        if tau_max <= tau_min + 1:
            raise ValueError(f"fmin {fmin!r} and fmax {fmax!r} at {self.sample_rate} Hz: the lags {tau_min} .. {tau_max} leave nothing to search")
        if tau_max > MAX_LAG:
            raise ValueError(f"fmin {fmin!r} at {self.sample_rate} Hz: the longest lag {tau_max} is above {MAX_LAG}")
        thr = _f32_finite("threshold", threshold)
        if not 0.0 < float(np.float32(thr)) <= 1.0:
            raise ValueError(f"threshold must be in (0, 1], not {threshold!r}")
        s(self, "threshold", thr)
        if not isinstance(center, (bool, np.bool_)):
            raise ValueError(f"center must be True or False, not {center!r}")
        s(self, "center", bool(center))
        if self.center:
            if align_length is not None:
                raise ValueError("align_length belongs to center=False")
        else:
            if align_length is None:
                raise ValueError("center=False needs align_length >= 1")
            align_length = _int("align_length", align_length, 1, (1 << 31) - 1)
        s(self, "align_length", align_length)
        s(self, "tau_min", tau_min)
        s(self, "tau_max", tau_max)

    @classmethod
    def like(cls, spec, **kw):
        """The Yin whose frames are those of `spec`, a features.LogMel, a cqt.ConstantQ, a stft.Spectrogram, a fbank.KaldiFbank or a mfcc.KaldiMfcc: its
        rate and hop, centred for a LogMel, a ConstantQ and a Spectrogram, align_length = spec.win_length for the Kaldi kinds (with snip_edges, the only Kaldi framing
        whose count this estimator has: ValueError without).  kw: the other arguments of `Yin`."""
        from .cqt import ConstantQ
        from .fbank import _KaldiFraming
        from .features import LogMel
        from .stft import Spectrogram

        if isinstance(spec, (LogMel, ConstantQ, Spectrogram)):
            return cls(spec.sample_rate, hop_length=spec.hop_length, center=True, **kw)
        if isinstance(spec, _KaldiFraming):
            if not spec.snip_edges:
                raise ValueError("a Kaldi transform with snip_edges=False reflects its last frames: no Yin has its frame count")
            return cls(spec.sample_rate, hop_length=spec.hop_length, center=False, align_length=spec.win_length, **kw)
        raise ValueError(f"spec must be a features.LogMel, a cqt.ConstantQ, a fbank.KaldiFbank or a mfcc.KaldiMfcc or a stft.Spectrogram, not {spec!r}")

    @property
    def span(self):
        """win_length + tau_max: the samples a frame reads"""
        return self.win_length + self.tau_max

    @property
    def first(self):
        """The first sample of frame 0: c_0 - span // 2 (negative: zeros are read)"""
        return (0 if self.center else self.align_length // 2) - self.span // 2

    def frames(self, L):
        """T' of a row of L samples (numpy arrays too)"""
        if self.center:
            return 1 + L // self.hop_length
        T = np.where(np.asarray(L) < self.align_length, 0, 1 + (np.asarray(L) - self.align_length) // self.hop_length)
        return int(T) if np.ndim(T) == 0 else T

    @property
    def min_frames(self):
        """The shortest row that has a frame"""
        return 0 if self.center else self.align_length

    def short(self, L):
        """What refuses a row of L < min_frames samples"""
        return f"num_frames {L}: a row of fewer than {self.min_frames} frames has no F0 frame"

    def lengths(self, lengths):
        """The frame count `frames` gives each length, -1 where a length is -1: an int64 torch tensor on the device of
        `lengths` for a tensor, an int64 numpy array for anything else"""
        try:
            import torch
        except ImportError:                                              # (the host specifications need no torch)
            torch = None
        if torch is not None and isinstance(lengths, torch.Tensor):
            if lengths.dtype.is_floating_point:
                raise ValueError("lengths must be integers")
            lens = lengths.to(torch.int64)
            if self.center:
                T = torch.div(lens, self.hop_length, rounding_mode="floor") + 1
            else:
                T = torch.where(lens < self.align_length, torch.zeros_like(lens),
                                1 + torch.div(lens - self.align_length, self.hop_length, rounding_mode="floor"))
            return torch.where(lens >= 0, T, torch.full_like(lens, -1))
        lens = np.asarray(lengths)
        if lens.dtype.kind not in "iu":
            raise ValueError("lengths must be integers")
        lens = lens.astype(np.int64)
        return np.where(lens >= 0, np.asarray(self.frames(np.maximum(lens, 0)), dtype=np.int64), -1)

    def voiced(self, y):
        """Which frames of y [..., 2, T'] (a tensor or an array, what `yin` and the host functions return) are voiced:
        ap < threshold, as a boolean [..., T']"""
        return y[..., 1, :] < float(np.float32(self.threshold))


def hz_to_cents(f0, ref):
    """1200 log2(f0 / ref): f0 (a tensor or an array) in cents above `ref` Hz"""
    return 1200.0 * (f0 / ref).log2() if hasattr(f0, "log2") else 1200.0 * np.log2(np.asarray(f0, dtype=np.float64) / ref)


def dprime_bound(spec):
    """E of the module: how far d' of any correct float32 evaluation is from the specification's, relatively"""
    return _gamma(2 * (spec.win_length + 2) + spec.tau_max + 2)


def f0_bound(spec, tau, kappa):
    """The relative bound of the module on f0 for a frame that chose `tau` with the parabola's kappa (arrays too); infinite
    where (E + 2 u) kappa is not below 1"""
    E = dprime_bound(spec) + 2 * _U
    eta = E * np.asarray(kappa, dtype=np.float64)
    with np.errstate(all="ignore"):
        S = np.where(eta < 1.0, np.where(eta > 0.0, eta / (1.0 - eta) + _U, 0.0), np.inf)
        return S / (np.asarray(tau, dtype=np.float64) - 0.5) + 3 * _U


def tile_frames(spec):
    """How many consecutive frames of a row one workgroup takes (alac_yin_tile of csrc/alac_yin.h): at most 8, fewer where
    their samples and their difference functions would not fit 8192 floats of LDS"""
    lags = spec.tau_max + 1
    room = LDS_FLOATS - 8 - spec.span - lags
    return int(max(1, min(TILE_MAX, 1 + room // (spec.hop_length + lags))))


def _host_args(x, spec, lengths):
    """x as [B, C, T] float32, whether it had its C, and v [B]"""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim not in (2, 3):
        raise ValueError(f"x must be float32 [B, C, T] or [B, T], not {x.dtype} {x.shape}")
    if not isinstance(spec, Yin):
        raise ValueError(f"spec must be a Yin, not {spec!r}")
    x3 = x if x.ndim == 3 else x[:, None, :]
    return x3, x.ndim == 3, _lengths_host("lengths", lengths, x.shape[0], x.shape[-1])


def _segments(row, v, spec, t0, t1, dtype, extra=0):
    """[t1 - t0, span + extra]: the samples frames t0 .. t1 of a row with v valid samples read, zeros outside [0, v)"""
    g = (spec.first + np.arange(t0, t1, dtype=np.int64)[:, None] * spec.hop_length
         + np.arange(spec.span + extra, dtype=np.int64)[None, :])
    inside = (g >= 0) & (g < v)
    return np.where(inside, row[np.clip(g, 0, max(len(row) - 1, 0))] if len(row) else 0, 0).astype(dtype)


def _rel(p, q):
    """|p - q| / (|p| + |q|), infinite for 0 / 0 (two zeros compare the same however they were computed) and for a NaN"""
    with np.errstate(all="ignore"):
        r = np.abs(p - q) / (np.abs(p) + np.abs(q))
    return np.where(np.isnan(r), np.inf, r)


def _choose(dp, c_last, spec, thr, rate, f, margin):
    """Steps 3 to 5 of a frame on d' [tau_max + 1] in the arithmetic `f` (np.float64 or np.float32): (f0, ap, tau, margin,
    kappa).  margin and kappa only with `margin` (else inf and 0)."""
    if c_last == 0:
        return f(0.0), f(1.0), 0, np.inf, 0.0
    lo, hi = spec.tau_min, spec.tau_max - 1                                  # the candidates lo .. hi
    m = np.inf
    cand = dp[lo:hi + 1]
    with np.errstate(all="ignore"):
        below = np.nonzero(cand < thr)[0]
        if len(below):
            tau = lo + int(below[0])
            if margin:
                seen = cand[:tau - lo + 1].astype(np.float64)
                r = np.abs(seen - float(thr)) / np.abs(seen)
                m = min(m, float(np.min(np.where(np.isnan(r), np.inf, r))))
            while tau + 1 <= hi:
                down = dp[tau + 1] < dp[tau]
                if margin:
                    m = min(m, float(_rel(np.float64(dp[tau + 1]), np.float64(dp[tau]))))
                if not down:
                    break
                tau += 1
        else:
            key = np.where(np.isnan(cand), np.inf, cand)
            tau = lo + int(np.argmin(key))
            if margin:
                r = np.abs(cand.astype(np.float64) - float(thr)) / np.abs(cand.astype(np.float64))
                m = min(m, float(np.min(np.where(np.isnan(r), np.inf, r))))
                others = np.delete(key, tau - lo).astype(np.float64)
                if len(others):
                    m = min(m, float(np.min(_rel(others, np.float64(key[tau - lo])))))
        a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
        n = f(a - c)
        q = f(f(a - f(2.0) * b) + c)
        kappa = 0.0
        if b <= a and b <= c and q > 0:
            shift = f(f(0.5) * n) / q
            shift = f(shift)
            if margin:
                kappa = float((np.float64(a) + 2.0 * np.float64(b) + np.float64(c)) / np.float64(q))
        else:
            shift = f(0.0)
        if margin:
            m = min(m, float(_rel(np.float64(b), np.float64(a))), float(_rel(np.float64(b), np.float64(c))))
        f0 = f(rate / f(f(tau) + shift))
    return f0, b, tau, m, kappa


def _dprime_f64(seg, spec):
    """Steps 1 and 2 of the specification on the frames' samples seg [F, span] float64: (d' [F, tau_max + 1], c[tau_max] [F])"""
    W = spec.win_length
    lag = np.arange(spec.tau_max + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.stack([np.sum((seg[:, :W] - seg[:, tau:tau + W]) ** 2, axis=1) for tau in range(spec.tau_max + 1)], axis=1)
        c = np.cumsum(d[:, 1:], axis=1)
        dp = np.ones_like(d)
        dp[:, 1:] = np.where(c == 0, 1.0, d[:, 1:] * lag[1:] / np.where(c == 0, 1.0, c))
    return dp, c[:, -1]


def yin_host(x, spec, lengths=None, margin=False):
    """The specification in numpy: float64 [B, C, 2, T'] ([B, 2, T'] for x [B, T]) from x float32, float64 arithmetic on the
    float32 input and on the float32 values of the threshold and the rate.  lengths: [B] integers (below 0 counts as 0, above
    T as T); default: T.  margin=True: returns (y, tau int64 [B, C, T'] -- the chosen lag, 0 for a silent frame and behind
    the row's frames --, margin float64 [B, C, T'], kappa float64 [B, C, T']) as the module defines them; the margin is
    infinite where a frame makes no choice."""
    x3, had_c, lens = _host_args(x, spec, lengths)
    B, C, T = x3.shape
    n = int(spec.frames(T))
    y = np.zeros((B, C, 2, n))
    taus = np.zeros((B, C, n), dtype=np.int64)
    margins = np.full((B, C, n), np.inf)
    kappas = np.zeros((B, C, n))
    thr, rate = np.float64(np.float32(spec.threshold)), np.float64(np.float32(spec.sample_rate))
    for b in range(B):
        v = int(lens[b])
        count = min(int(spec.frames(v)), n)
        for ch in range(C):
            if count == 0:
                continue
            dp, last = _dprime_f64(_segments(x3[b, ch], v, spec, 0, count, np.float64), spec)
            for t in range(count):
                f0, ap, tau, m, k = _choose(dp[t], last[t], spec, thr, rate, np.float64, margin)
                y[b, ch, 0, t], y[b, ch, 1, t], taus[b, ch, t], margins[b, ch, t], kappas[b, ch, t] = f0, ap, tau, m, k
    if not had_c:
        y, taus, margins, kappas = y[:, 0], taus[:, 0], margins[:, 0], kappas[:, 0]
    return (y, taus, margins, kappas) if margin else y


def _scan64(d):
    """c [F, tau_max] float32 from d [F, tau_max] (the lags 1 .. tau_max) in the kernel's order: see the module"""
    F, n = d.shape
    K = (n + 63) // 64
    v = np.zeros((F, K * 64), dtype=np.float32)
    v[:, :n] = d
    v = v.reshape(F, K, 64)
    for h in (1, 2, 4, 8, 16, 32):
        w = v.copy()
        w[:, :, h:] = (v[:, :, h:] + v[:, :, :-h]).astype(np.float32)
        v = w
    c = np.empty_like(v)
    carry = np.zeros(F, dtype=np.float32)
    for k in range(K):
        c[:, k, :] = (carry[:, None] + v[:, k, :]).astype(np.float32)
        carry = c[:, k, 63]
    return c.reshape(F, K * 64)[:, :n], carry


def _dprime_f32(seg, spec):
    """Steps 1 and 2 in the kernel's arithmetic on the frames' samples seg [F, span] float32: (d' [F, tau_max + 1], c[tau_max] [F])"""
    f32 = np.float32
    W, L = spec.win_length, spec.tau_max + 1
    lag = np.arange(L).astype(f32)
    acc = np.zeros((seg.shape[0], L), dtype=f32)
    with np.errstate(all="ignore"):
        for j in range(W):
            e = (seg[:, j, None] - seg[:, j:j + L]).astype(f32)
            acc = _fma32(e, e, acc)
        c, last = _scan64(acc[:, 1:])
        dp = np.ones_like(acc)
        dp[:, 1:] = np.where(c != 0, ((acc[:, 1:] * lag[1:]).astype(f32) / np.where(c != 0, c, f32(1))).astype(f32), f32(1))
    return dp, last


def yin_host_f32(x, spec, lengths=None, tile=None, taus=False):
    """The kernel's arithmetic in numpy, bit for bit: float32 [B, C, 2, T'] ([B, 2, T'] for x [B, T]).  tile: how many frames
    are evaluated together (default `tile_frames(spec)`, the kernel's): every frame is its own, so it changes nothing.
    taus=True: returns (y, the chosen lags int64 [B, C, T'])."""
    x3, had_c, lens = _host_args(x, spec, lengths)
    f32 = np.float32
    B, C, T = x3.shape
    n = int(spec.frames(T))
    tile = tile_frames(spec) if tile is None else _int("tile", tile, 1)
    y = np.zeros((B, C, 2, n), dtype=f32)
    chosen = np.zeros((B, C, n), dtype=np.int64)
    thr, rate = f32(spec.threshold), f32(spec.sample_rate)
    for b in range(B):
        v = int(lens[b])
        count = min(int(spec.frames(v)), n)
        for ch in range(C):
            for t0 in range(0, count, tile):
                t1 = min(t0 + tile, count)
                dp, last = _dprime_f32(_segments(x3[b, ch], v, spec, t0, t1, f32), spec)
                for t in range(t0, t1):
                    f0, ap, tau, _, _ = _choose(dp[t - t0], last[t - t0], spec, thr, rate, f32, False)
                    y[b, ch, 0, t], y[b, ch, 1, t], chosen[b, ch, t] = f0, ap, tau
    if not had_c:
        y, chosen = y[:, 0], chosen[:, 0]
    return (y, chosen) if taus else y


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _yin(ctx, pcm, spec, lengths, out):
    """`yin` behind its first check, on pcm [B, C, T]; ctx() gives the context that runs it (the corpus's own inside
    `Corpus.crops`); out: a contiguous float32 tensor [B, C, 2, T'] to write, or None for a new one"""
    import torch

    if not isinstance(spec, Yin):
        raise ValueError(f"spec must be a Yin, not {spec!r}")
    stride = _planes("pcm", pcm)
    B, C, T = pcm.shape
    n = int(spec.frames(T))
    shape = (B, C, 2, n)
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    d_valid = _lengths_device("lengths", lengths, B, pcm.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    else:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != pcm.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {pcm.device}")
        if pcm.numel() and out.numel():
            (x0, x1), o0 = _span(pcm, stride), out.data_ptr()
            if x0 < o0 + 4 * out.numel() and o0 < x1:
                raise ValueError("out overlaps pcm")
    if out.numel() == 0:
        return out
    if T == 0:                       # (centred: one frame a row, of silence; the library takes no empty planes)
        out[:, :, 0, :] = 0.0
        out[:, :, 1, :] = 1.0
        return out
    with torch.cuda.device(pcm.device):
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        ctx().yin_device(pcm, B, C, stride, T, d_valid, spec.sample_rate, spec.win_length, spec.hop_length, spec.tau_min, spec.tau_max,
                         0 if spec.center else spec.align_length, spec.threshold, out, n, stream=stream)
    return out


def yin(pcm, spec, lengths=None, out=None):
    """The F0 contour on the GPU: pcm float32 [B, C, T] or [B, T] on the device, contiguous or the slice [..., :T] of a
    contiguous tensor (what `load`, `load_batch` and `crops` return; what lies behind the slice is not read); spec: a `Yin`;
    lengths: [B] integers, a sequence or a tensor (as `crops` returns them; -1 counts as 0, more than T as T); default: T.
    Returns float32 [B, C, 2, T'] ([B, 2, T'] for [B, T]), T' = spec.frames(T): f0 in Hz and the aperiodicity, zeros at and
    behind the row's frame count (see the module).  out: a contiguous tensor of that shape apart from pcm; default: a new
    one.  One launch, asynchronous on the current stream, nothing is read back; ValueError before any device work."""
    import torch

    ctx = _device_context("pcm", pcm, "[B, C, T] or [B, T]")
    if pcm.dim() == 2:
        if out is not None and (not isinstance(out, torch.Tensor) or out.dim() != 3):
            raise ValueError("out must be a contiguous float32 tensor [B, 2, T']")
        res = _yin(ctx, pcm[:, None, :], spec, lengths, None if out is None else out[:, None])
        return res[:, 0]
    return _yin(ctx, pcm, spec, lengths, out)
