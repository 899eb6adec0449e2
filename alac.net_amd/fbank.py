"""Kaldi filterbank features behind the decode: framing, the frame's mean, pre-emphasis, window, DFT, power, mel projection
and log in one kernel (alacgpu_fbank_device, csrc/alac_fbank.hip).  What Kaldi's `compute-fbank-feats`,
torchaudio.compliance.kaldi.fbank, lhotse and the recipes built on them compute; `features.LogMel` is the torch.stft / Whisper
front end and cannot express it.

Lengths are in samples: Kaldi's 25 ms and 10 ms at 16 kHz are win_length 400 and hop_length 160.  A row is x[0 .. L) float32,
L >= 1.  n_fft is win_length rounded up to a power of two (or win_length itself with round_to_power_of_two=False),
n_bins = n_fft // 2 + 1.

Frames.
    snip_edges=True    T' = 0 for L < win_length, else 1 + (L - win_length) // hop; frame t starts at g0 = t * hop
    snip_edges=False   T' = (L + hop // 2) // hop; frame t starts at g0 = t * hop + hop // 2 - win_length // 2, and an index g
                       outside 0 .. L is reflected as Kaldi's loop does (-g - 1 below 0, 2 L - 1 - g at or behind L, repeated
                       until it is inside): m = g mod 2 L (floored), then m if m < L, else 2 L - 1 - m.  Rows shorter than
                       half a window are reflected several times.

Per frame, in this order, N = win_length, n < N, g = g0 + n:
    s[n] = scale * x[g]                                     (exact for a power of two: 32768 is Kaldi's int16 scale)
    mu   = (sum of s) / N,  d[n] = s[n] - mu                (remove_dc_offset)
    y[n] = d[n] - c * d[n - 1],  y[0] = d[0] - c * d[0]     (preemphasis c != 0; c is used as its float32 value)
    a[n] = window[n] * y[n]
    X[j] = sum over n of a[n] * basis[n, j],  j < 2 * n_bins
    P[k] = X[k]^2 + X[n_bins + k]^2                         (its square root with use_power=False)
    M[m] = sum over k of fb[m, k] * P[k]
    out[m, t] = ln(max(M[m], 2^-23))                        (log=True; FLT_EPSILON is Kaldi's floor)  or  M[m]  (log=False)

    window[i]            povey (0.5 - 0.5 cos(2 pi i / (N - 1)))^0.85, hanning 0.5 - 0.5 cos(2 pi i / (N - 1)), hamming
                         0.54 - 0.46 cos(2 pi i / (N - 1)), blackman 0.42 - 0.5 cos(2 pi i / (N - 1)) + 0.08 cos(4 pi i / (N - 1)),
                         rectangular 1
    basis[n, k]          = cos(2 pi ((n k) mod n_fft) / n_fft),  basis[n, n_bins + k] = -sin(the same),  n < N: the zeros that
                         pad a frame to n_fft have no rows
    fb                   = kaldi_mel_banks(...): triangles that are linear on the mel axis mel(f) = 1127 ln(1 + f / 700)

Each table is built in float64 and rounded to float32 once.  The layout is the project's, [..., n_mels, T']: Kaldi's matrix
(frames by bins) transposed, so `MeanVar` per mel bin and `SpecAugment` work behind it as behind `LogMel` features.

The kernel's float32 order (`fbank_host_f32` follows the kernel, never the other way round).  s is rounded once.  The sum of a
frame is eight partial sums, partial j over the taps n = j, j + 8, j + 16 ... in ascending n from zero, added as the tree
((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)); mu is that sum divided by N, correctly rounded; d is one subtraction.  y is
ONE fused multiply-add, fma(-c, d[n - 1], d[n]); a is one product; X[j] is a chain of fused multiply-adds in ascending n from
zero (the exact-f32 matrix instruction), P = fma(re, re, round(im * im)), its root correctly rounded, M[m] a chain of fused
multiply-adds in ascending k from zero.  With u = 2^-24 a float32 evaluation in that order stays within

    e_s   = u |s|
    e_mu  = (N / 8 + 6) u (sum of |s|) / N + (sum of e_s) / N
    e_d   = e_s + e_mu + u |d|                               (e_s without remove_dc_offset)
    e_y   = e_d[n] + c e_d[n - 1] + u |y|                    (e_d without pre-emphasis)
    e_a   = window[n] e_y + u |a|
    E_j   = sum over n of e_a[n] |basis[n, j]|
    delta_j = E_j + (1 + 2^-10) u (N E_j + sum over k < N of |S_k[j]|),  S_k[j] = sum over n <= k of a[n] basis[n, j]
            (every fused multiply-add of the chain rounds once, by at most u times its result, a partial sum of the frame
            as rounded; the bound is of the chain in ascending n and of no other order)
    dP_k  = 2 |Re| delta_re + delta_re^2 + 2 |Im| delta_im + delta_im^2 + 3 u P_k
            (use_power=False: sqrt(P + dP) - sqrt(max(P - dP, 0)) + 2 u sqrt(P + dP) in its place)
    dM_m  = sum over k of fb[m, k] dP_k + (n_bins + 1) u M_m

of the exact value; `fbank_host(..., bound=True)` returns dM.

Input that is not finite follows IEEE arithmetic and is never hidden.  A NaN at sample i reaches exactly the frames that
contain i (after the reflection), and all of those, whatever the window's weight there: the frame's mean carries it to every
tap (without remove_dc_offset the window's zero weights at both ends do, 0 * NaN being NaN).  Every other frame is bit for bit
what it is without it.  max(M, floor) keeps a NaN, as np.maximum and torch.clamp do.

Out of scope: `dither` (Kaldi draws it per frame element; there is nothing to hold a device generator to, and torchaudio's
and lhotse's default is 0), `use_energy` and `raw_energy` (mfcc.KaldiMfcc has them: here they would change the transform's
line count), `htk_compat` and VTLN.  MFCCs are mfcc.py's, on this module's framing, window and banks; deltas are deltas.py's.

`kaldi_window`, `kaldi_mel_banks`, `KaldiFbank`, `fbank_host` and `fbank_host_f32` need no device.  `fbank` is the call on
device tensors.
"""
import numpy as np

from ._stageargs import _f32_finite
from .features import _chain, _int, _on_device, _Transform, dft_basis  # noqa: F401 (_chain: the twin's, once)

MIN_WIN, MAX_WIN, MAX_NFFT, MAX_MELS = 16, 2048, 2048, 256
FLOOR = 2.0 ** -23                                              # FLT_EPSILON
WINDOWS = ("povey", "hanning", "hamming", "blackman", "rectangular")
MEAN_PARTIALS = 8                                               # the partial sums of a frame's mean
FLAG_SNIP_EDGES, FLAG_REMOVE_DC, FLAG_USE_POWER, FLAG_LOG = 1, 2, 4, 8      # alacgpu_fbank_device's flags
_U = 2.0 ** -24


def kaldi_mel(f):
    """1127 ln(1 + f / 700) (float64 arrays too)"""
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def kaldi_window(name, win_length):
    """Kaldi's window of that name (see the module), float32 [win_length], computed in float64 and rounded once"""
    N = _int("win_length", win_length, 2)
    if name not in WINDOWS:
        raise ValueError(f"window must be one of {', '.join(WINDOWS)}, not {name!r}")
    a = 2.0 * np.pi * np.arange(N, dtype=np.float64) / (N - 1)
    if name == "povey":
        w = (0.5 - 0.5 * np.cos(a)) ** 0.85
    elif name == "hanning":
        w = 0.5 - 0.5 * np.cos(a)
    elif name == "hamming":
        w = 0.54 - 0.46 * np.cos(a)
    elif name == "blackman":
        w = 0.42 - 0.5 * np.cos(a) + 0.08 * np.cos(2.0 * a)
    else:
        w = np.ones(N)
    return w.astype(np.float32)


def _kaldi_band(sample_rate, low_freq, high_freq):
    low, high = float(low_freq), float(high_freq)
    high = sample_rate / 2.0 + high if high <= 0.0 else high
    if not (0.0 <= low < high <= sample_rate / 2.0):
        raise ValueError(f"0 <= low_freq < high <= sample_rate / 2 does not hold for low_freq = {low}, high = {high}, "
                         f"sample_rate = {sample_rate}")
    return low, high


def kaldi_mel_banks(sample_rate, n_fft, n_mels, low_freq=20.0, high_freq=0.0):
    """Kaldi's mel banks, float32 [n_mels, n_fft // 2 + 1], computed in float64 and rounded once: n_mels triangles, linear
    on the mel axis, over n_mels + 2 points equally spaced in mel between low_freq and high (sample_rate / 2 + high_freq for
    high_freq <= 0, else high_freq); bin k < n_fft // 2 at z = mel(k * sample_rate / n_fft) weighs (z - left) / (centre - left)
    for left < z <= centre, (right - z) / (right - centre) for centre < z < right.  The Nyquist bin weighs 0; no
    normalisation.  ValueError: limits as `KaldiFbank`'s."""
    sample_rate = _int("sample_rate", sample_rate, 1)
    n_fft = _int("n_fft", n_fft, MIN_WIN, MAX_NFFT)
    n_mels = _int("n_mels", n_mels, 1, MAX_MELS)
    low, high = _kaldi_band(sample_rate, low_freq, high_freq)
    mel_low, mel_high = float(kaldi_mel(low)), float(kaldi_mel(high))
    delta = (mel_high - mel_low) / (n_mels + 1)
    left = (mel_low + np.arange(n_mels, dtype=np.float64) * delta)[:, None]
    centre, right = left + delta, left + 2.0 * delta
    z = kaldi_mel(np.arange(n_fft // 2, dtype=np.float64) * (sample_rate / n_fft))[None, :]
    rise, fall = (z - left) / (centre - left), (right - z) / (right - centre)
    w = np.where((z > left) & (z <= centre), rise, np.where((z > centre) & (z < right), fall, 0.0))
    fb = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float64)
    fb[:, :n_fft // 2] = w
    return fb.astype(np.float32)


def fbank_basis(win_length, n_fft):
    """`features.dft_basis` with win_length rows: float32 [win_length, 2 * n_bins]"""
    return dft_basis(n_fft, win_length)


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, not {v!r}")
    return bool(v)


def _kaldi_fields(sample_rate, win_length, hop_length, n_mels, low_freq, high_freq, preemphasis, window, scale, **flags):
    """What `KaldiFbank` and mfcc.KaldiMfcc check and build alike: ((window, basis, fb), the fields of `_Transform._freeze`
    but n_mels); `flags`: the transform's switches by name, each True or False.  ValueError as `KaldiFbank` states."""
    sample_rate = _int("sample_rate", sample_rate, 1)
    win_length = _int("win_length", win_length, MIN_WIN, MAX_WIN)
    hop_length = _int("hop_length", hop_length, 1, win_length)
    n_mels = _int("n_mels", n_mels, 1, MAX_MELS)
    flags = {n: _flag(n, v) for n, v in flags.items()}
    n_fft = 1 << (win_length - 1).bit_length() if flags["round_to_power_of_two"] else win_length
    if n_fft > MAX_NFFT:
        raise ValueError(f"n_fft = {n_fft} is above {MAX_NFFT}")
    low_freq, high_freq = float(low_freq), float(high_freq)
    _kaldi_band(sample_rate, low_freq, high_freq)
    if isinstance(preemphasis, (bool, np.bool_)) or not isinstance(preemphasis, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(preemphasis) <= 1.0:
        raise ValueError(f"preemphasis must be a number of 0 .. 1, not {preemphasis!r}")
    preemphasis = float(np.float32(preemphasis))
    scale = float(np.float32(_f32_finite("scale", scale)))
    if scale == 0.0:
        raise ValueError("scale must not be zero in float32")
    tables = (kaldi_window(window, win_length), fbank_basis(win_length, n_fft),
              kaldi_mel_banks(sample_rate, n_fft, n_mels, low_freq, high_freq))
    return tables, dict(sample_rate=sample_rate, win_length=win_length, hop_length=hop_length, n_fft=n_fft, n_bins=n_fft // 2 + 1,
                        low_freq=low_freq, high_freq=high_freq, preemphasis=preemphasis, window_type=window, scale=scale, **flags)


class _KaldiFraming:
    """Kaldi's framing as `Corpus.crops` and `_on_device` ask a transform for it: what `KaldiFbank` and mfcc.KaldiMfcc share
    beside their tables"""

    __slots__ = ()

    def frames(self, L):
        """T' of a row of L samples (numpy arrays too)"""
        if self.snip_edges:
            T = np.where(np.asarray(L) < self.win_length, 0, 1 + (np.asarray(L) - self.win_length) // self.hop_length)
        else:
            T = (np.asarray(L) + self.hop_length // 2) // self.hop_length
        return int(T) if np.ndim(T) == 0 else T

    @property
    def min_frames(self):
        """The shortest row that has a frame"""
        return self.win_length if self.snip_edges else self.hop_length - self.hop_length // 2

    def short(self, L):
        """What refuses a row of L < min_frames samples"""
        return f"num_frames {L}: a row of fewer than {self.min_frames} frames has no feature frame"

    def lengths(self, lengths):
        """`fbank_lengths(lengths, self)`"""
        return fbank_lengths(lengths, self)


class KaldiFbank(_KaldiFraming, _Transform):
    """An immutable description of Kaldi's fbank transform (see the module) together with its three float32 tables: `window`
    [win_length], `basis` [win_length, 2 * n_bins] and `fb` [n_mels, n_bins] (read-only arrays).  Lengths are in samples:
    Kaldi's frame_length 25 ms and frame_shift 10 ms at 16 kHz are win_length 400 and hop_length 160.  The features are
    [..., n_mels, T']: Kaldi's matrix transposed.  ValueError unless 16 <= win_length <= 2048, 1 <= hop_length <= win_length,
    1 <= n_mels <= 256, n_fft <= 2048, 0 <= low_freq < high <= sample_rate / 2, 0 <= preemphasis <= 1, scale finite and not
    zero in float32, a window of `WINDOWS`."""

    __slots__ = ("sample_rate", "win_length", "hop_length", "n_mels", "n_fft", "n_bins", "low_freq", "high_freq", "preemphasis",
                 "remove_dc_offset", "window_type", "round_to_power_of_two", "snip_edges", "use_power", "log", "scale")

    def __init__(self, sample_rate, win_length=400, hop_length=160, n_mels=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97,
                 remove_dc_offset=True, window="povey", round_to_power_of_two=True, snip_edges=True, use_power=True, log=True,
                 scale=32768.0):
        tables, fields = _kaldi_fields(sample_rate, win_length, hop_length, n_mels, low_freq, high_freq, preemphasis, window, scale,
                                       remove_dc_offset=remove_dc_offset, round_to_power_of_two=round_to_power_of_two,
                                       snip_edges=snip_edges, use_power=use_power, log=log)
        self._freeze(*tables, n_mels=tables[2].shape[0], **fields)

    def __repr__(self):
        return (f"KaldiFbank(sample_rate={self.sample_rate}, win_length={self.win_length}, hop_length={self.hop_length}, "
                f"n_mels={self.n_mels}, n_fft={self.n_fft}, window={self.window_type!r}, snip_edges={self.snip_edges}, "
                f"preemphasis={self.preemphasis}, log={self.log})")

    @property
    def flags(self):
        """alacgpu_fbank_device's flags: 1 snip_edges, 2 remove_dc_offset, 4 use_power, 8 log"""
        return (FLAG_SNIP_EDGES * self.snip_edges | FLAG_REMOVE_DC * self.remove_dc_offset | FLAG_USE_POWER * self.use_power |
                FLAG_LOG * self.log)

    def launch(self, gpu, src, rows, channels, src_stride, L, out, stream):
        """The features of src (float32 device tensor, planar [rows, channels, src_stride], the first L of a plane are signal)
        into out [rows, channels, n_mels, frames(L)] by the AlacGpuContext `gpu`: one alacgpu_fbank_device call on `stream`"""
        window, basis, fb = self.device_tables(src.device)
        gpu.fbank_device(src, rows, channels, src_stride, L, self.win_length, self.n_fft, self.hop_length, self.n_mels, window,
                         basis, fb, self.flags, self.preemphasis, self.scale, out, self.frames(L), stream=stream)


def fbank_frame_index(L, spec):
    """idx int64 [T', win_length]: the sample frame t's tap n reads, after the reflection of snip_edges=False"""
    T = spec.frames(int(L))
    first = 0 if spec.snip_edges else spec.hop_length // 2 - spec.win_length // 2
    g = np.arange(T, dtype=np.int64)[:, None] * spec.hop_length + first + np.arange(spec.win_length, dtype=np.int64)[None, :]
    if not spec.snip_edges:
        m = np.mod(g, 2 * L)                                         # floored
        g = np.where(m < L, m, 2 * L - 1 - m)
    return g


def _rows_of(x, spec, kind=None):
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    if x.ndim < 1 or x.shape[-1] < 1:
        raise ValueError(f"x must be [..., L] with L >= 1, not {x.shape}")
    if not isinstance(spec, kind or KaldiFbank):
        raise ValueError(f"spec must be a {(kind or KaldiFbank).__name__}")
    return x, x.shape[-1]


def _prev(v):
    """v[:, n - 1], v[:, 0] its own predecessor"""
    return np.concatenate([v[:, :1], v[:, :-1]], axis=1)


def _row_f64(row, idx, spec, bound):
    """One row of `fbank_host` (row float64 [L], idx `fbank_frame_index`), and what mfcc.mfcc_host needs of it beside M: returns
    (M [T', n_mels], dM or None, d, a, e_d, e_a) -- d [T', N] the frames after scale and mean, a the windowed frames, e_d and
    e_a how far a float32 evaluation may be from them (the module's e_d and e_a; None without bound)"""
    N, n_bins, c = spec.win_length, spec.n_bins, spec.preemphasis
    w = spec.window.astype(np.float64)[None, :]
    basis = spec.basis.astype(np.float64)
    fb = spec.fb.astype(np.float64)
    T = idx.shape[0]
    s = spec.scale * row[idx]                                        # [T, N]
    d = s - s.sum(axis=1, keepdims=True) / N if spec.remove_dc_offset else s
    y = d - c * _prev(d) if c != 0.0 else d
    a = w * y
    X = a @ basis
    P = X[:, :n_bins] ** 2 + X[:, n_bins:] ** 2
    dM = e_d = e_a = None
    if bound:
        e = _U * np.abs(s)
        if spec.remove_dc_offset:
            e_mu = (N / 8 + 6) * _U * np.abs(s).sum(axis=1, keepdims=True) / N + e.sum(axis=1, keepdims=True) / N
            e = e + e_mu + _U * np.abs(d)
        e_d = e
        if c != 0.0:
            e = e + c * _prev(e) + _U * np.abs(y)
        e_a = e = w * e + _U * np.abs(a)
        E = e @ np.abs(basis)
        chain = np.empty_like(X)
        for t in range(T):                                           # the partial sums of frame t's chains, [N, 2 n_bins]
            chain[t] = np.abs(np.cumsum(a[t][:, None] * basis, axis=0)).sum(axis=0)
        delta = E + (1 + 2.0 ** -10) * _U * (N * E + chain)
        dre, dim = delta[:, :n_bins], delta[:, n_bins:]
        dP = 2 * np.abs(X[:, :n_bins]) * dre + dre ** 2 + 2 * np.abs(X[:, n_bins:]) * dim + dim ** 2 + 3 * _U * P
        if not spec.use_power:
            dP = np.sqrt(P + dP) - np.sqrt(np.maximum(P - dP, 0.0)) + 2 * _U * np.sqrt(P + dP)
    if not spec.use_power:
        P = np.sqrt(P)
    M = P @ fb.T                                                     # [T, n_mels]
    if bound:
        dM = dP @ fb.T + (n_bins + 1) * _U * M
    return M, dM, d, a, e_d, e_a


def fbank_host(x, spec, bound=False):
    """The kernel's specification in numpy: x float32 [..., L], L >= 1, to float64 [..., n_mels, T'] -- float64 arithmetic on
    the float32 input and the float32 tables, scale and preemphasis of `spec`.  bound=True: returns (out, dM), dM float64 like
    out: how far a float32 evaluation in the kernel's order may be from M (the module docstring's bound; in the domain of M,
    whatever spec.log is)."""
    x, L = _rows_of(x, spec)
    idx = fbank_frame_index(L, spec)
    T = idx.shape[0]
    rows = x.reshape(-1, L).astype(np.float64)
    out = np.empty((rows.shape[0], spec.n_mels, T), dtype=np.float64)
    dM = np.empty_like(out) if bound else None
    for r, row in enumerate(rows):
        M, dM_r = _row_f64(row, idx, spec, bound)[:2]
        if bound:
            dM[r] = dM_r.T
        out[r] = (np.log(np.maximum(M, FLOOR)) if spec.log else M).T
    out = out.reshape(x.shape[:-1] + (spec.n_mels, T))
    return (out, dM.reshape(out.shape)) if bound else out


def _row_f32(row, idx, spec):
    """One row of `fbank_host_f32` (row float32 [L]), and what mfcc.mfcc_host_f32 needs of it beside M: returns (M float32
    [T', n_mels], d, a) -- d [T', N] the frames after scale and mean, a the windowed frames, as the kernel rounds them"""
    f32, f64 = np.float32, np.float64
    N, n_bins = spec.win_length, spec.n_bins
    c, scale = f32(spec.preemphasis), f32(spec.scale)
    T = idx.shape[0]
    basis = spec.basis.astype(f64)
    fbT = np.ascontiguousarray(spec.fb.astype(f64).T)
    s = (scale * row[idx]).astype(f32)                               # [T, N]
    d = s
    if spec.remove_dc_offset:
        part = np.zeros((T, MEAN_PARTIALS), dtype=f32)
        for n in range(N):                                           # partial n % 8 takes tap n, ascending
            part[:, n % MEAN_PARTIALS] += s[:, n]
        p = part
        while p.shape[1] > 1:                                        # neighbours first: ((p0 + p1) + (p2 + p3)) + ...
            p = p[:, 0::2] + p[:, 1::2]
        mu = (p / f32(N)).astype(f32)                                # [T, 1]
        d = (s - mu).astype(f32)
    y = d
    if spec.preemphasis != 0.0:                                      # fma(-c, d[n - 1], d[n]): the product is exact in float64
        y = (d.astype(f64) - f64(c) * _prev(d).astype(f64)).astype(f32)
    a = (spec.window[None, :] * y).astype(f32)
    X = _chain(a, basis)
    re, im = X[:, :n_bins].astype(f64), X[:, n_bins:].astype(f64)
    P = (re * re + (im * im).astype(f32).astype(f64)).astype(f32)
    if not spec.use_power:
        P = np.sqrt(P)                                               # float32, correctly rounded
    return _chain(P, fbT), d, a


def fbank_host_f32(x, spec):
    """The kernel's arithmetic in numpy, one float32 operation at a time in the order the module states: x float32 [..., L] to
    float32 [..., n_mels, T'] (with spec.log the log is numpy's float32 one, not the device's logf).  Its distance from
    `fbank_host` is what a correct float32 evaluation costs: the tests hold the kernel to a small multiple of that, far
    inside dM."""
    x, L = _rows_of(x, spec)
    idx = fbank_frame_index(L, spec)
    T = idx.shape[0]
    rows = x.reshape(-1, L)
    out = np.empty((rows.shape[0], spec.n_mels, T), dtype=np.float32)
    for r, row in enumerate(rows):
        M = _row_f32(row, idx, spec)[0]
        if spec.log:
            M = np.log(np.maximum(M, np.float32(FLOOR)))
        out[r] = M.T
    return out.reshape(x.shape[:-1] + (spec.n_mels, T))


def fbank_lengths(lengths, spec):
    """The frame count `spec.frames` gives each length, -1 where a length is -1: an int64 torch tensor on the device of
    `lengths` for a tensor, an int64 numpy array for anything else"""
    win, hop = spec.win_length, spec.hop_length
    try:
        import torch
    except ImportError:                                              # (the host specifications need no torch)
        torch = None
    if torch is not None and isinstance(lengths, torch.Tensor):
        if lengths.dtype.is_floating_point:
            raise ValueError("lengths must be integers")
        lens = lengths.to(torch.int64)
        if spec.snip_edges:
            T = torch.where(lens < win, torch.zeros_like(lens), 1 + torch.div(lens - win, hop, rounding_mode="floor"))
        else:
            T = torch.div(lens + hop // 2, hop, rounding_mode="floor")
        return torch.where(lens >= 0, T, torch.full_like(lens, -1))
    lens = np.asarray(lengths)
    if lens.dtype.kind not in "iu":
        raise ValueError("lengths must be integers")
    lens = lens.astype(np.int64)
    return np.where(lens >= 0, np.asarray(spec.frames(np.maximum(lens, 0)), dtype=np.int64), -1)


# ---- on the device -------------------------------------------------------------------------------------------------------------
def fbank(pcm, spec, lengths=None):
    """Kaldi fbank features on the GPU: pcm float32 [..., T] on the device (as `load`, `load_batch` and `crops` return it),
    T >= 1, to float32 [..., spec.n_mels, spec.frames(T)]; one kernel, asynchronous on the current stream.  Every row is
    transformed over its whole T.  A T that gives no frame gives an empty tensor and no launch.  lengths (a sequence or an
    integer tensor): returns (features, `fbank_lengths` of them as an int64 tensor where `lengths` was)."""
    takes = "[..., T], T >= 1"
    short = lambda T: f"pcm must be a float32 device tensor {takes}" if T < 1 else None
    return _on_device(pcm, spec, KaldiFbank, takes, short, lengths)
