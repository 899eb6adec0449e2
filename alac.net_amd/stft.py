"""Linear, complex and banded (mel) spectrograms behind the decode: framing, window, an FFT, power or magnitude, an optional
banded filterbank and the log in one kernel (alacgpu_stft_device, csrc/alac_stft.hip).

Spectrogram(sample_rate, n_fft = N, hop_length = hop, win_length, window, power, filterbank, log, floor):  N is 256, 512, 1024
or 2048, n_bins = K = N / 2 + 1.  A row is x[0 .. L) float32 with L >= N / 2 + 1.  The framing is `features.LogMel`'s exactly
(`features.frame_index`; torch.stft's center=True, pad_mode="reflect"): frame t of 0 .. T', T' = 1 + L // hop, is centred on
sample t hop,

    x_t[n]    = x[t hop - N / 2 + n],  n < N, reflected once about 0 and about L
    w[n]      = the window of win_length taps at offset (N - win_length) // 2 of the N, zeros around it (as torch.stft places
                it): the periodic Hann window 0.5 - 0.5 cos(2 pi n / win_length), float64 rounded once, or the caller's
    X_t[k]    = sum over n of w[n] x_t[n] exp(-2 pi i k n / N),   k < K
    power     None: the complex spectrum, 2 K lines: Re X in the lines 0 .. K, Im X behind them (`as_complex` puts them together)
              2: |X|^2,   1: |X|,   K lines
    filterbank  fb float32 [lines <= 256, K] on the power or the magnitude: M[m] = sum over k of fb[m, k] v[k]
    out       v or M, or with log="ln" | "log10" the log of max(., floor); a NaN stays a NaN

What lies behind a crop's length is the zeros `crops` wrote: the transform sees the padded row, as `LogMel` does.

The tables.  `window` [N] as above; `table` [N, 2], (cos, -sin)(2 pi k / N) in float64 rounded once (`pitch.twiddles`); of a
filterbank, per line, `bands` int32 [lines, 3]: (first, count, offset) -- the span from the line's first to its last weight
that is not zero, and where the span's weights begin in `weights`, the spans packed in the order of the lines (one zero stands
behind the last, so that the array is never empty).  A mel triangle is a short band; a dense row is a band of K and still
correct; a row of zeros has count 0 and gives 0 in front of the floor.  `fb` is the filterbank itself.

The evaluation order -- what the kernel does, and `spectrogram_host_f32` operation by operation; every operation is one IEEE
float32 operation, rounded once:

    pairs     the frames 2 j and 2 j + 1 of a plane are one pair -- by the frame's parity in the row, never by a tile --:
              z[n] = (w[n] * x_2j[n], w[n] * x_2j+1[n]); if T' is odd the last frame's partner is zero, not a product.
    transform the phase vocoder's forward transform of N points (`pitch._forward`: a radix-2 stage for 512 and 2048, radix-4
              stages; 256 is pure radix-4), bin k at `pitch.positions(N)[k]`.
    unpack    for k = 0 .. N / 2, with Z[N] = Z[0]:
                  A.re = 0.5 * (Z.re[k] + Z.re[N - k])       A.im = 0.5 * (Z.im[k] - Z.im[N - k])        frame 2 j
                  B.re = 0.5 * (Z.im[k] + Z.im[N - k])       B.im = 0.5 * (Z.re[N - k] - Z.re[k])        frame 2 j + 1
              each sum rounded once (the halving is exact but for underflow).
    power     P = fma(re, re, round(im * im)); the root is the correctly rounded one.
    filterbank  acc = fma(weights[offset + i], v[first + i], acc) for i = 0 .. count - 1 from zero.
    log       max(v, floor) keeps a NaN; the logarithm is the device's logf or log10f (the twin's is the float64 one rounded:
              without a log the twin equals the kernel bit for bit, behind one they differ by the logarithm's last places).

The bound, derived, not measured (`spectrogram_host(..., bound=True)` returns it per element), the way `pitch.analyse_bound`
and `cqt.cqt_host(bound=True)` derive theirs.  u = 2^-24, gamma_n = n u / (1 - n u).  The pair's products carry u each.  The
transform: a radix-4 stage is two radix-2 stages of which one has exact twiddles, so Higham's Theorem 24.2 for s = log2 N
radix-2 stages covers it: the computed Z is within f sqrt(N) ||z||_2 of the exact one in the 2-norm, f = s eta / (1 - s eta),
eta = u + gamma_4 (sqrt(2) + u) (`pitch._fft_factor`), so every element of Z, real or imaginary part, is within

    e    = (f + u (1 + f)) sqrt(N) ||z||_2,      ||z||_2^2 = ||w x_2j||^2 + ||w x_2j+1||^2

of the exact value.  The unpacking halves a sum of two such parts and rounds it once:

    d_re = e + u (|re| + e),   d_im likewise                                  (the complex lines' bound)
    D    = 2 |re| d_re + d_re^2 + 2 |im| d_im + d_im^2,   dP = D + 3 u (P + D)           (the square, the fma's two roundings)
    dv   = dP for power=2;  min(dP / sqrt(P), sqrt(dP)) + u (sqrt(P) + that) for power=1
    dM   = sum over the band of |fb| dv + gamma_count sum of |fb| (v + dv)                 (the chain of `count` fmas)
    dout = dv or dM, or for a log:  max(log(max(v + dv, floor)) - log(vf), log(vf) - log(max(v - dv, floor))) + 4 u |log(vf)|,
           vf = max(v, floor), which leaves a float32 logarithm two units in the last place

It assumes that nothing underflows.  It is a normwise bound handed to every element: e is the whole pair's, so a bin far below
the frame's level has a bound far above its own rounding; tests/test_stft_spec.py prints its median relative size.

Input that is not finite follows IEEE arithmetic and is never hidden.  A transform mixes every tap of its pair: a NaN or an
infinity at sample i can reach every element of the two frames of any pair of which one frame has a tap on i -- the partner
frame too, and a tap whose window weight is zero too, 0 * inf being NaN -- and no element of any other pair, which is bit for
bit what it is without it.  max(v, floor) keeps a NaN.

`Spectrogram`, `spectrogram_host`, `spectrogram_host_f32`, `transform_host_f32`, `tile_frames` and `as_complex` need no
device; `spectrogram` is the call on device tensors.  A `Spectrogram(filterbank=mel_filterbank(...), log="ln")` is a
`LogMel` of the same shape by another algorithm: n log n work and no basis table, where `LogMel` is a DFT as a GEMM; their
results agree within the two bounds, not bit for bit.
Out of scope: another n_fft (400 stays `LogMel`'s), the inverse transform as a public call, center=False, other padding
modes, autograd, moving `LogMel` onto the FFT.
"""
import math

import numpy as np

from . import pitch
from .cqt import _fma
from .features import _LOGS, _int, _on_device, _Transform, feature_lengths, frame_index

N_FFTS = (256, 512, 1024, 2048)
MAX_LINES = 256                                                # ALAC_STFT_MAX_LINES of csrc/alac_stft.h
_LDS_SHARE = 80 << 10                                          # ALAC_STFT_LDS_SHARE
_POWERS = {None: 0, 1: 1, 2: 2}
_U = 2.0 ** -24


def _gamma(k):
    return k * _U / (1.0 - k * _U)


def tile_frames(n_fft, lines, filterbank):
    """How many consecutive frames of a plane one workgroup takes (alac_stft_tile of csrc/alac_stft.h): 32768 / n_fft, at most
    64, halved once where that brings z, the tile [lines][tile + 1] and, with a filterbank, v from above to at or below 80 KiB"""
    lds = lambda tile: 8 * n_fft + 4 * lines * (tile + 1) + (8 * (n_fft // 2 + 1) if filterbank else 0)
    cap = min(32768 // n_fft, 64)
    return cap // 2 if lds(cap) > _LDS_SHARE and lds(cap // 2) <= _LDS_SHARE else cap


class Spectrogram(_Transform):
    """An immutable description of a short-time Fourier transform (see the module) with its tables: `window` float32 [n_fft],
    `table` float32 [n_fft, 2], and of a filterbank `fb` float32 [lines, n_bins], `bands` int32 [lines, 3] and `weights`
    float32 (read-only arrays; `fb` is None and the other two are empty without one).  hop_length: default n_fft // 4;
    win_length: default n_fft; window: the caller's float32 [win_length] instead of the periodic Hann window; power: 2, 1 or
    None (the complex spectrum); filterbank: None or [1 .. 256, n_bins] (`mel_filterbank(...)`); log: "ln", "log10" or None
    (floor is then ignored).  `n_mels` is the line count `Corpus.crops`, `Deltas`, `MeanVar` and `SpecAugment` see of a
    transform: n_bins, the filterbank's rows, or 2 n_bins for power=None.  ValueError unless n_fft is 256, 512, 1024 or 2048,
    1 <= hop_length <= n_fft, 1 <= win_length <= n_fft, the window is win_length finite numbers, the filterbank is finite,
    power is 2, 1 or None, floor > 0 and finite; power=None takes neither a filterbank nor a log."""

    __slots__ = ("table", "bands", "weights", "sample_rate", "n_fft", "hop_length", "win_length", "n_bins", "n_mels", "power", "log",
                 "floor")
    _TABLES = ("window", "table", "bands", "weights")

    def __init__(self, sample_rate, n_fft=1024, hop_length=None, win_length=None, window=None, power=2, filterbank=None, log=None,
                 floor=1e-10):
        sample_rate = _int("sample_rate", sample_rate, 1, (1 << 31) - 1)
        if isinstance(n_fft, (bool, np.bool_)) or not isinstance(n_fft, (int, np.integer)) or int(n_fft) not in N_FFTS:
            raise ValueError(f"n_fft must be one of {N_FFTS}, not {n_fft!r}")
        n_fft = int(n_fft)
        n_bins = n_fft // 2 + 1
        hop_length = _int("hop_length", n_fft // 4 if hop_length is None else hop_length, 1, n_fft)
        win_length = _int("win_length", n_fft if win_length is None else win_length, 1, n_fft)
        if isinstance(power, (bool, np.bool_)) or (power is not None and power not in (1, 2)):
            raise ValueError(f"power must be 2, 1 or None, not {power!r}")
        power = None if power is None else int(power)
        if log not in _LOGS:
            raise ValueError(f"log must be 'ln', 'log10' or None, not {log!r}")
        floor = float(floor)
        if not (floor > 0.0 and math.isfinite(floor) and math.isfinite(float(np.float32(floor))) and float(np.float32(floor)) > 0.0):
            raise ValueError(f"floor must be positive and finite in float32, not {floor!r}")
        if power is None and (filterbank is not None or log is not None):
            raise ValueError("power=None is the complex spectrum: it takes neither a filterbank nor a log")
        if window is None:
            taps = pitch.window(win_length, np.float32)
        else:
            taps = np.array(window, dtype=np.float32, order="C")
            if taps.shape != (win_length,) or not np.isfinite(taps).all():
                raise ValueError(f"window must be {win_length} finite numbers, not {taps.shape}")
        w = np.zeros(n_fft, dtype=np.float32)
        at = (n_fft - win_length) // 2
        w[at:at + win_length] = taps
        if filterbank is None:
            fb, lines = None, (n_bins if power is not None else 2 * n_bins)
            bands, weights = np.zeros((0, 3), dtype=np.int32), np.zeros(1, dtype=np.float32)
        else:
            fb = np.array(filterbank, dtype=np.float32, order="C")
            if fb.ndim != 2 or fb.shape[1] != n_bins or not 1 <= fb.shape[0] <= MAX_LINES or not np.isfinite(fb).all():
                raise ValueError(f"filterbank must be finite [1 .. {MAX_LINES}, {n_bins}], not {fb.shape}")
            lines = fb.shape[0]
            bands, packed = np.zeros((lines, 3), dtype=np.int32), []
            for m in range(lines):
                nz = np.flatnonzero(fb[m])
                first, count = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if len(nz) else (0, 0)
                bands[m] = first, count, sum(len(p) for p in packed)
                packed.append(fb[m, first:first + count])
            weights = np.concatenate(packed + [np.zeros(1, dtype=np.float32)]).astype(np.float32)
            fb.flags.writeable = False
        cos, msin = pitch.twiddles(n_fft)
        self._freeze(w, None, fb, table=np.ascontiguousarray(np.stack([cos, msin], axis=1)), bands=bands, weights=weights,
                     sample_rate=sample_rate, n_fft=n_fft, hop_length=hop_length, win_length=win_length, n_bins=n_bins, n_mels=lines,
                     power=power, log=log, floor=floor)

    def __repr__(self):
        return (f"Spectrogram(sample_rate={self.sample_rate}, n_fft={self.n_fft}, hop_length={self.hop_length}, "
                f"win_length={self.win_length}, power={self.power}, lines={self.n_mels}, log={self.log!r}, floor={self.floor})")

    @property
    def log_mode(self):
        """alacgpu_stft_device's log_mode: 0 none, 1 ln, 2 log10"""
        return _LOGS[self.log]

    @property
    def power_mode(self):
        """alacgpu_stft_device's power: 0 the complex spectrum, 1 magnitude, 2 power"""
        return _POWERS[self.power]

    @property
    def tile(self):
        """`tile_frames` of this transform"""
        return tile_frames(self.n_fft, self.n_mels, self.fb is not None)

    def frames(self, L):
        """T' = 1 + L // hop_length (numpy arrays too)"""
        return 1 + L // self.hop_length

    @property
    def min_frames(self):
        """The shortest row the transform takes: n_fft // 2 + 1"""
        return self.n_fft // 2 + 1

    def short(self, L):
        """What refuses a row of L < min_frames samples"""
        return f"num_frames {L}: the transform needs more than n_fft // 2 = {self.n_fft // 2}"

    def lengths(self, lengths):
        """`feature_lengths(lengths, hop_length)`"""
        return feature_lengths(lengths, self.hop_length)

    def launch(self, gpu, src, rows, channels, src_stride, L, out, stream):
        """The spectrogram of src (float32 device tensor, planar [rows, channels, src_stride], the first L of a plane are
        signal) into out [rows, channels, n_mels, frames(L)] by the AlacGpuContext `gpu`: one alacgpu_stft_device call on `stream`"""
        window, table, bands, weights = self.device_tables(src.device)
        fb = self.fb is not None
        gpu.stft_device(src, rows, channels, src_stride, L, self.n_fft, self.hop_length, window, table, self.power_mode,
                        self.bands if fb else None, bands if fb else None, weights if fb else None, self.log_mode, self.floor, out,
                        self.frames(L), stream=stream)


def as_complex(feats):
    """The complex spectrum of a power=None `Spectrogram`'s output: a float32 tensor [..., 2 n_bins, T'] to torch.complex64
    [..., n_bins, T'], the lines 0 .. n_bins the real parts, those behind them the imaginary parts"""
    import torch

    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or feats.dim() < 2 or feats.shape[-2] % 2:
        raise ValueError("feats must be a float32 tensor [..., 2 n_bins, T']")
    K = feats.shape[-2] // 2
    return torch.complex(feats[..., :K, :].contiguous(), feats[..., K:, :].contiguous())


# ---- the specification and the twin ------------------------------------------------------------------------------------------------
def _args(x, spec):
    x = np.asarray(x)
    if not isinstance(spec, Spectrogram):
        raise ValueError(f"spec must be a Spectrogram, not {spec!r}")
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    L = x.shape[-1] if x.ndim else 0
    if x.ndim < 1 or L <= spec.n_fft // 2:
        raise ValueError(f"x must be [..., L] with L > n_fft // 2 = {spec.n_fft // 2}, not {x.shape}")
    return x, L


def _log(spec):
    return np.log if spec.log == "ln" else np.log10


def spectrogram_host(x, spec, bound=False):
    """The kernel's specification in numpy: x float32 [..., L], L > n_fft // 2, to float64 [..., lines, T'] -- np.fft.rfft of the
    framed, windowed rows, float64 arithmetic on the float32 input and the float32 tables of `spec`.  bound=True: returns
    (out, dout), dout float64 like out: how far a float32 evaluation in the module's order may be from out (the module
    docstring's bound)."""
    x, L = _args(x, spec)
    N, K = spec.n_fft, spec.n_bins
    idx, _ = frame_index(L, N, spec.hop_length)                                        # (n_fft is even: every tap is inside)
    T = idx.shape[0]
    rows = x.reshape(-1, L).astype(np.float64)
    w = spec.window.astype(np.float64)
    floor = float(np.float32(spec.floor))
    with np.errstate(all="ignore"):
        fr = rows[:, idx] * w                                                           # [R, T, N]
        X = np.fft.rfft(fr, axis=-1)                                                    # [R, T, K]
        re, im = X.real, X.imag
        if bound:
            n2 = (fr ** 2).sum(axis=-1)                                                 # [R, T]
            Tp = (T + 1) // 2
            both = np.zeros((rows.shape[0], 2 * Tp))
            both[:, :T] = n2
            both = both.reshape(-1, Tp, 2).sum(axis=-1)                                 # the pair's ||z||^2
            f = pitch._fft_factor(N)
            e = ((f + _U * (1 + f)) * math.sqrt(N) * np.sqrt(both)).repeat(2, axis=1)[:, :T, None]
            dre, dim = e + _U * (np.abs(re) + e), e + _U * (np.abs(im) + e)
        if spec.power is None:
            v = np.concatenate([re, im], axis=-1)
            dv = np.concatenate([dre, dim], axis=-1) if bound else None
        else:
            P = re ** 2 + im ** 2
            v = np.sqrt(P) if spec.power == 1 else P
            if bound:
                D = 2 * np.abs(re) * dre + dre ** 2 + 2 * np.abs(im) * dim + dim ** 2
                dP = D + 3 * _U * (P + D)
                if spec.power == 1:
                    dv = np.where(P > 0, np.minimum(dP / np.where(P > 0, np.sqrt(P), 1.0), np.sqrt(dP)), np.sqrt(dP))
                    dv = dv + _U * (v + dv)
                else:
                    dv = dP
            if spec.fb is not None:
                fb = np.abs(spec.fb.astype(np.float64))
                if bound:
                    dv = dv @ fb.T + _gamma(spec.bands[:, 1].astype(np.float64)) * ((np.abs(v) + dv) @ fb.T)
                v = v @ spec.fb.astype(np.float64).T
            if spec.log is not None:
                lg = _log(spec)
                vf = np.maximum(v, floor)
                if bound:
                    hi, lo = lg(np.maximum(v + dv, floor)), lg(np.maximum(v - dv, floor))
                    dv = np.maximum(hi - lg(vf), lg(vf) - lo) + 4 * _U * np.abs(lg(vf))
                v = lg(vf)
    shape = x.shape[:-1] + (spec.n_mels, T)
    out = np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(shape)
    return (out, np.ascontiguousarray(dv.transpose(0, 2, 1)).reshape(shape)) if bound else out


def transform_host_f32(zr, zi, table=None):
    """The kernel's transform of pairs in numpy float32: zr, zi float32 [n, N] (copied) to (Zr, Zi) float32 [n, N] in natural
    order: `pitch._forward`, read at `pitch.positions(N)`.  table: (cos, -sin) float32 [N] each instead of `pitch.twiddles(N)`."""
    zr, zi = np.array(zr, dtype=np.float32, order="C"), np.array(zi, dtype=np.float32, order="C")
    N = zr.shape[1]
    with np.errstate(all="ignore"):
        pitch._forward(zr, zi, pitch.twiddles(N) if table is None else table)
    pos = pitch.positions(N)
    return zr[:, pos], zi[:, pos]


def spectrogram_host_f32(x, spec, table=None, unpack_sign=1.0):
    """The kernel's arithmetic in numpy, one float32 operation at a time (the module's evaluation order): x float32 [..., L] to
    float32 [..., lines, T'].  Without a log it equals the kernel bit for bit; its logarithm is the float64 one rounded.
    table and unpack_sign are for the tests that show the bound is not vacuous: another twiddle table, and the sign of the
    second term of B.re."""
    x, L = _args(x, spec)
    f32 = np.float32
    N, K = spec.n_fft, spec.n_bins
    idx, _ = frame_index(L, N, spec.hop_length)
    T = idx.shape[0]
    Tp = (T + 1) // 2
    rows = x.reshape(-1, L)
    R = rows.shape[0]
    half = f32(0.5)
    with np.errstate(all="ignore"):
        fr = np.zeros((R, 2 * Tp, N), dtype=f32)                                        # (a lone last frame's partner: zeros)
        fr[:, :T] = rows[:, idx] * spec.window
        fr = fr.reshape(R * Tp, 2, N)
        Zr, Zi = transform_host_f32(fr[:, 0], fr[:, 1], table)
        k = np.arange(K)
        nk = (N - k) % N
        are, aim = half * (Zr[:, k] + Zr[:, nk]), half * (Zi[:, k] - Zi[:, nk])
        bre, bim = half * (Zi[:, k] + f32(unpack_sign) * Zi[:, nk]), half * (Zr[:, nk] - Zr[:, k])
        re = np.stack([are, bre], axis=1).reshape(R, 2 * Tp, K)[:, :T]                  # [R, T, K]
        im = np.stack([aim, bim], axis=1).reshape(R, 2 * Tp, K)[:, :T]
        if spec.power is None:
            v = np.concatenate([re, im], axis=-1)
        else:
            v = _fma(re, re, (im * im).astype(f32))
            if spec.power == 1:
                v = np.sqrt(v)                                                          # (numpy's float32 root is the correctly rounded one)
            if spec.fb is not None:
                first, count, off = (spec.bands[:, c].astype(np.int64) for c in range(3))
                flat = v.reshape(R * T, K)
                acc = np.zeros((R * T, spec.n_mels), dtype=f32)
                for i in range(int(count.max())):
                    on = np.flatnonzero(count > i)                                      # the lines that have a weight here: no other is touched
                    acc[:, on] = _fma(spec.weights[off[on] + i][None, :], flat[:, first[on] + i], acc[:, on])
                v = acc.reshape(R, T, spec.n_mels)
            if spec.log is not None:
                v = np.maximum(v, f32(spec.floor))
                v = _log(spec)(v.astype(np.float64)).astype(f32)
    return np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(x.shape[:-1] + (spec.n_mels, T))


# ---- on the device -------------------------------------------------------------------------------------------------------------
def spectrogram(pcm, spec, lengths=None):
    """The spectrogram on the GPU: pcm float32 [..., T] on the device (as `load`, `load_batch` and `crops` return it),
    T > n_fft // 2, to float32 [..., spec.n_mels, 1 + T // hop]; one kernel, asynchronous on the current stream.  Every row is
    transformed over its whole T (what lies behind a file's or a crop's length is the zeros the decode wrote).  lengths (a
    sequence or an integer tensor): returns (features, lengths // hop + 1 as an int64 tensor where `lengths` was; an entry of
    -1 stays -1)."""
    def short(T):
        if T <= spec.n_fft // 2:
            return f"T = {T} frames: the transform needs more than n_fft // 2 = {spec.n_fft // 2}"

    return _on_device(pcm, spec, Spectrogram, "[..., T]", short, lengths)
