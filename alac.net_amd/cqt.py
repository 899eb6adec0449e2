"""Constant-Q features behind the decode: the direct (Brown 1991 / nnAudio CQT1992v2) constant-Q transform, every bin's own
kernel against the signal, magnitude or power, and the log, in one kernel (alacgpu_cqt_device, csrc/alac_cqt.hip).

ConstantQ(sample_rate = sr, hop_length = hop, f_min, n_bins, bins_per_octave = bpo, filter_scale, scale, power, log, floor):

    Q      = filter_scale / (2^(1 / bpo) - 1)
    f_k    = f_min 2^(k / bpo),  k < n_bins                                  (`cqt_frequencies`)
    N_k    = ceil(Q sr / f_k)                                                 (`cqt_lengths`; non-increasing in k)
    c_k    = N_k // 2
    w_k[n] = 0.5 - 0.5 cos(2 pi n / N_k),  n < N_k                            the periodic Hann window
    s_k    = sqrt(N_k) if scale else 1
    g_k[n] = s_k w_k[n] exp(-2 pi i f_k (n - c_k) / sr) / sum over n of w_k[n]

A row is x[0 .. L) float32, L >= 1, and zero outside: nothing is reflected (librosa's pad_mode="constant"; what `yin` does).
Frame t of 0 .. T', T' = 1 + L // hop, is centred on sample t hop:

    C[k, t]   = sum over n < N_k of g_k[n] x[t hop - c_k + n]
    P[k, t]   = Re(C)^2 + Im(C)^2
    v[k, t]   = sqrt(P) for power=1, P for power=2
    out[k, t] = v, or with log="ln" | "log10" the log of max(v, floor)

What lies behind a crop's length is the zeros `crops` wrote, so every row has a frame: `min_frames` is 1.  Only magnitudes
leave the kernel: the phase origin c_k is a convention nobody observes.  With the defaults (C1, 84 bins, 12 an octave) at
22 050 Hz N_0 = 11 339 and N_83 = 94; at 44 100 Hz N_0 = 22 678; 252 bins at 36 an octave have N_0 = 34 683.

The tables: the real and imaginary parts of every g_k, built in float64 (the phase f_k (n - c_k) / sr reduced to a fraction of
a turn first) and rounded to float32 once.  They are stored as the kernel reads them, `table`: the bins in blocks of
BLOCK_BINS = 16 neighbours, a block as [K_b][32] floats, K_b the even number at or above the block's longest length N_{16 b},
row r of the 32 the real ((r >> 3) & 1 == 0) or imaginary part of the block's bin (r >> 4) 8 + (r & 7), and bin k's taps at
n' = c_{16 b} - c_k + n of the K_b: centred, zeros around them.  `ConstantQ.kernel(k)` is g_k out of that table.  `lens` is
the N_k.  Doubling sr and f_min changes no table.

The kernel evaluates this in float32: Re and Im are each a chain of fused multiply-adds fma(g[n], x[.], acc) in ascending n
from zero (on the MFMA, whose zeros in front of and behind a bin's taps add nothing to a chain of finite values),
P = fma(re, re, round(im im)), and the root is the correctly rounded one.  With u = 2^-24 and gamma_N = N u / (1 - N u) any
such evaluation stays within

    d_re = gamma_{N_k} sum over n of |Re g_k[n]| |x[.]|,   d_im likewise
    D    = 2 |Re| d_re + d_re^2 + 2 |Im| d_im + d_im^2
    dP   = D + 3 u (P + D)
    dv   = dP for power=2;  min(dP / sqrt(P), sqrt(dP)) + u (sqrt(P) + that) for power=1
    dout = dv, or for a log:  max(log(max(v + dv, floor)) - log(vf), log(vf) - log(max(v - dv, floor))) + 4 u |log(vf)|,
           vf = max(v, floor), which leaves a float32 logarithm two units in the last place

of the exact value; `cqt_host(..., bound=True)` returns dout.  `cqt_host_f32` is the kernel operation by operation, and
equals it bit for bit without a log; its logarithm is the float64 one rounded, which the device's logf and log10f (one and
two units in the last place) do not always match.

Input that is not finite follows IEEE arithmetic and is never hidden.  A NaN at sample i reaches element (k, t) exactly when
i is one of bin k's own N_k taps of frame t -- the tap n = 0 too, whose window weight is zero -- and every other element,
the same frame's shorter bins included, is bit for bit what it is without the NaN: the support is per bin, not per frame.
An infinity likewise (0 inf and inf - inf are NaN; where the sums do give an infinity, P is +inf).  max(v, floor) keeps a NaN.
The kernel keeps this although a block's bins share zero-padded taps: a tile whose span holds a value that is not finite is
evaluated bin by bin over each bin's own taps, in the same order, so the elements out of the value's reach keep their bits.

`ConstantQ`, `cqt_host`, `cqt_host_f32`, `cqt_frequencies`, `cqt_lengths`, `cqt_work` and `tile_frames` need no device; `cqt`
is the call on device tensors.
"""
import math

import numpy as np

from ._stageargs import _f32_finite, _fma32
from .features import _LOGS, _int, _on_device, _Transform, feature_lengths

# ALAC_CQT_BLOCK_BINS, ALAC_CQT_TILE, ALAC_CQT_MAX_TAPS, ALAC_CQT_MAX_BINS, ALAC_CQT_LDS_FLOATS of csrc/alac_cqt.h
BLOCK_BINS, TILE, MAX_TAPS, MAX_BINS, LDS_FLOATS = 16, 32, 36864, 512, 40832
MAX_BINS_PER_OCTAVE, MAX_HOP, MAX_FILTER_SCALE = 96, 1 << 20, 16.0
C1_HZ = 32.70319566257483
_U = 2.0 ** -24


def _gamma(k):
    return k * _U / (1.0 - k * _U)


def _fma(x, y, z):
    """`_fma32`, and IEEE's answer where the exact sum is not finite (an infinite or NaN operand), which `_fma32`'s rounding
    does not take"""
    with np.errstate(all="ignore"):
        plain = np.asarray(x, dtype=np.float32).astype(np.float64) * np.asarray(y, dtype=np.float32).astype(np.float64) + np.asarray(z, dtype=np.float32).astype(np.float64)
        return np.where(np.isfinite(plain), _fma32(x, y, z), plain.astype(np.float32))


def _lengths(sample_rate, f_min, n_bins, bins_per_octave, filter_scale):
    """(f_k float64 [n_bins], N_k int64 [n_bins])"""
    Q = filter_scale / (2.0 ** (1.0 / bins_per_octave) - 1.0)
    f = f_min * 2.0 ** (np.arange(n_bins, dtype=np.float64) / bins_per_octave)
    return f, np.ceil(Q * sample_rate / f).astype(np.int64)


def _blocks(N):
    """The layout of `table` for the lengths N: per block of BLOCK_BINS bins (K_b, the block's offset in floats, where its
    taps begin in a frame's span: c_0 - c_{16 b}), and the floats of the whole table"""
    out, off = [], 0
    for first in range(0, len(N), BLOCK_BINS):
        K = (int(N[first]) + 1) & ~1
        out.append((K, off, int(N[0]) // 2 - int(N[first]) // 2))
        off += 32 * K
    return out, off


def _rows(j):
    """The rows of a block's bin j < 16: (real, imaginary)"""
    r = (j >> 3) * 16 + (j & 7)
    return r, r + 8


def tile_frames(n0, hop):
    """How many consecutive frames of a plane one workgroup takes (alac_cqt_tile of csrc/alac_cqt.h): 32, fewer where their
    span, (tile - 1) hop + n0 + 1 samples (and one float of skew per hop for an even hop), would not fit 40832 floats of LDS"""
    n0e = n0 + 1
    for tile in range(TILE, 1, -1):
        span = (tile - 1) * hop + n0e
        if span + (0 if hop & 1 else (span - 1) // hop + 1) <= LDS_FLOATS:
            return tile
    return 1


class ConstantQ(_Transform):
    """An immutable description of a constant-Q transform (see the module) with its tables: `table`, float32, the kernels in
    the kernel's blocked layout, and `lens`, int32 [n_bins], the N_k (read-only arrays).  `n_mels` is n_bins: the line count
    `Corpus.crops`, `Deltas`, `MeanVar` and `SpecAugment` see of a transform.  log: "ln", "log10" or None (floor is then
    ignored).  ValueError unless 1 <= n_bins <= 512, 1 <= bins_per_octave <= 96, 1 <= hop_length <= 2^20, 0 < filter_scale
    <= 16, f_min > 0, the highest bin's frequency is below sample_rate / 2, the shortest kernel has two taps, the longest at
    most MAX_TAPS = 36864 (what the kernel's span of LDS holds), power is 1 or 2, floor > 0 and finite."""

    __slots__ = ("table", "lens", "sample_rate", "hop_length", "f_min", "n_bins", "n_mels", "bins_per_octave", "filter_scale", "scale",
                 "power", "log", "floor")
    _TABLES = ("table", "lens")

    def __init__(self, sample_rate, hop_length=512, f_min=C1_HZ, n_bins=84, bins_per_octave=12, filter_scale=1.0, scale=True,
                 power=1.0, log=None, floor=1e-10):
        sample_rate = _int("sample_rate", sample_rate, 1, (1 << 31) - 1)
        hop_length = _int("hop_length", hop_length, 1, MAX_HOP)
        n_bins = _int("n_bins", n_bins, 1, MAX_BINS)
        bins_per_octave = _int("bins_per_octave", bins_per_octave, 1, MAX_BINS_PER_OCTAVE)
        f_min = _f32_finite("f_min", f_min)
        filter_scale = _f32_finite("filter_scale", filter_scale)
        if not f_min > 0.0:
            raise ValueError(f"f_min must be positive, not {f_min!r}")
        if not 0.0 < filter_scale <= MAX_FILTER_SCALE:
            raise ValueError(f"filter_scale must be in (0, {MAX_FILTER_SCALE}], not {filter_scale!r}")
        if not isinstance(scale, (bool, np.bool_)):
            raise ValueError(f"scale must be True or False, not {scale!r}")
        if isinstance(power, (bool, np.bool_)) or power not in (1, 2):
            raise ValueError(f"power must be 1 or 2, not {power!r}")
        if log not in _LOGS:
            raise ValueError(f"log must be 'ln', 'log10' or None, not {log!r}")
        floor = float(floor)
        if not (floor > 0.0 and math.isfinite(floor) and math.isfinite(float(np.float32(floor))) and float(np.float32(floor)) > 0.0):
            raise ValueError(f"floor must be positive and finite in float32, not {floor!r}")
        f, N = _lengths(sample_rate, f_min, n_bins, bins_per_octave, filter_scale)
        if not f[-1] < sample_rate / 2.0:
            raise ValueError(f"bin {n_bins - 1} at {f[-1]:.6g} Hz is not below sample_rate / 2 = {sample_rate / 2.0}")
        if N[-1] < 2:
            raise ValueError(f"filter_scale {filter_scale!r}: the shortest kernel has {int(N[-1])} taps, fewer than 2")
        if N[0] > MAX_TAPS:
            raise ValueError(f"the longest kernel has {int(N[0])} taps: the kernel's span holds at most {MAX_TAPS}")
        blocks, floats = _blocks(N)
        table = np.zeros(floats, dtype=np.float32)
        for k in range(n_bins):
            Nk = int(N[k])
            K, off, _ = blocks[k // BLOCK_BINS]
            n = np.arange(Nk, dtype=np.float64)
            w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / Nk)
            turn = (f[k] / sample_rate) * (n - Nk // 2)
            ang = 2.0 * np.pi * (turn - np.rint(turn))
            amp = (math.sqrt(Nk) if scale else 1.0) * w / np.sum(w)
            blk = table[off:off + 32 * K].reshape(K, 32)
            at = int(N[k - k % BLOCK_BINS]) // 2 - Nk // 2
            re, im = _rows(k % BLOCK_BINS)
            blk[at:at + Nk, re] = amp * np.cos(ang)
            blk[at:at + Nk, im] = -amp * np.sin(ang)
        self._freeze(None, None, None, table=table, lens=N.astype(np.int32), sample_rate=sample_rate, hop_length=hop_length, f_min=f_min,
                     n_bins=n_bins, n_mels=n_bins, bins_per_octave=bins_per_octave, filter_scale=filter_scale, scale=bool(scale),
                     power=int(power), log=log, floor=floor)

    def __repr__(self):
        return (f"ConstantQ(sample_rate={self.sample_rate}, hop_length={self.hop_length}, f_min={self.f_min}, n_bins={self.n_bins}, "
                f"bins_per_octave={self.bins_per_octave}, filter_scale={self.filter_scale}, scale={self.scale}, power={self.power}, "
                f"log={self.log!r}, floor={self.floor})")

    @property
    def log_mode(self):
        """alacgpu_cqt_device's log_mode: 0 none, 1 ln, 2 log10"""
        return _LOGS[self.log]

    def kernel(self, k):
        """(Re g_k, Im g_k): float32 [N_k] each, out of `table`"""
        k = _int("k", k, 0, self.n_bins - 1)
        N = self.lens
        K, off, _ = _blocks(N)[0][k // BLOCK_BINS]
        at = int(N[k - k % BLOCK_BINS]) // 2 - int(N[k]) // 2
        blk = self.table[off:off + 32 * K].reshape(K, 32)[at:at + int(N[k])]
        re, im = _rows(k % BLOCK_BINS)
        return blk[:, re], blk[:, im]

    def frames(self, L):
        """T' = 1 + L // hop_length (numpy arrays too)"""
        return 1 + L // self.hop_length

    @property
    def min_frames(self):
        """The shortest row the transform takes: 1"""
        return 1

    def short(self, L):
        """What refuses a row of L < min_frames samples"""
        return f"num_frames {L}: the transform needs a sample"

    def lengths(self, lengths):
        """`feature_lengths(lengths, hop_length)`: lengths // hop + 1, and -1 stays -1"""
        return feature_lengths(lengths, self.hop_length)

    def launch(self, gpu, src, rows, channels, src_stride, L, out, stream):
        """The features of src (float32 device tensor, planar [rows, channels, src_stride], the first L of a plane are signal)
        into out [rows, channels, n_bins, frames(L)] by the AlacGpuContext `gpu`: one alacgpu_cqt_device call on `stream`"""
        table, lens = self.device_tables(src.device)
        gpu.cqt_device(src, rows, channels, src_stride, L, self.hop_length, self.n_bins, self.lens, lens, table, self.power, self.log_mode,
                       self.floor, out, self.frames(L), stream=stream)


def cqt_frequencies(spec):
    """f_k, float64 [n_bins]"""
    return _lengths(spec.sample_rate, spec.f_min, spec.n_bins, spec.bins_per_octave, spec.filter_scale)[0]


def cqt_lengths(spec):
    """N_k, int64 [n_bins]"""
    return spec.lens.astype(np.int64)


def cqt_work(spec):
    """(sum of N_k, the multiply-add rows the kernel's tiling issues per frame): a block of 16 bins runs all of its 16 over
    the K_b of its longest kernel, so the second number is the sum over the blocks of 16 K_b.  (The dense form, every kernel
    padded to 16384 taps, issues 16384 n_bins.)"""
    N = cqt_lengths(spec)
    return int(N.sum()), int(sum(BLOCK_BINS * K for K, _, _ in _blocks(N)[0]))


def _args(x, spec):
    x = np.asarray(x)
    if not isinstance(spec, ConstantQ):
        raise ValueError(f"spec must be a ConstantQ, not {spec!r}")
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    if x.ndim < 1 or x.shape[-1] < 1:
        raise ValueError(f"x must be [..., L] with L >= 1, not {x.shape}")
    return x, x.shape[-1]


def _taps(rows, T, hop, ck, Nk, dtype):
    """[R, T, Nk]: the samples bin k's taps read in every frame of every row, zeros outside the row"""
    L = rows.shape[1]
    g = np.arange(T, dtype=np.int64)[:, None] * hop - ck + np.arange(Nk, dtype=np.int64)[None, :]
    inside = (g >= 0) & (g < L)
    return np.where(inside[None], rows[:, np.where(inside, g, 0)], 0).astype(dtype)


def cqt_host(x, spec, bound=False):
    """The kernel's specification in numpy: x float32 [..., L], L >= 1, to float64 [..., n_bins, T'] -- float64 arithmetic on
    the float32 input and the float32 tables of `spec`.  bound=True: returns (out, dout), dout float64 like out: how far a
    float32 evaluation in the module's order may be from out (the module docstring's bound)."""
    x, L = _args(x, spec)
    T = int(spec.frames(L))
    rows = x.reshape(-1, L)
    out = np.empty((rows.shape[0], spec.n_bins, T), dtype=np.float64)
    d = np.empty_like(out) if bound else None
    floor = float(np.float32(spec.floor))
    with np.errstate(all="ignore"):
        for k in range(spec.n_bins):
            Nk = int(spec.lens[k])
            g = np.stack(spec.kernel(k), axis=1).astype(np.float64)                   # [Nk, 2]
            fr = _taps(rows, T, spec.hop_length, Nk // 2, Nk, np.float64)             # [R, T, Nk]
            C = fr @ g                                                                # [R, T, 2]
            P = C[..., 0] ** 2 + C[..., 1] ** 2
            v = np.sqrt(P) if spec.power == 1 else P
            if bound:
                dc = _gamma(Nk) * (np.abs(fr) @ np.abs(g))
                D = 2 * np.abs(C[..., 0]) * dc[..., 0] + dc[..., 0] ** 2 + 2 * np.abs(C[..., 1]) * dc[..., 1] + dc[..., 1] ** 2
                dP = D + 3 * _U * (P + D)
                if spec.power == 1:
                    dv = np.where(P > 0, np.minimum(dP / np.where(P > 0, np.sqrt(P), 1.0), np.sqrt(dP)), np.sqrt(dP))
                    dv = dv + _U * (v + dv)
                else:
                    dv = dP
            if spec.log is not None:
                lg = np.log if spec.log == "ln" else np.log10
                vf = np.maximum(v, floor)
                if bound:
                    hi, lo = lg(np.maximum(v + dv, floor)), lg(np.maximum(v - dv, floor))
                    dv = np.maximum(hi - lg(vf), lg(vf) - lo) + 4 * _U * np.abs(lg(vf))
                v = lg(vf)
            out[:, k, :] = v
            if bound:
                d[:, k, :] = dv
    out = out.reshape(x.shape[:-1] + (spec.n_bins, T))
    return (out, d.reshape(out.shape)) if bound else out


def cqt_host_f32(x, spec):
    """The kernel's arithmetic in numpy, one float32 operation at a time: x float32 [..., L] to float32 [..., n_bins, T'].
    Re and Im: acc = fma(g[n], x[t hop - c_k + n], acc) for n = 0 .. N_k - 1 from zero, the fused multiply-add exact
    (`_fma`); P = fma(re, re, round(im im)); the root correctly rounded; max(v, floor) keeps a NaN; the logarithm is the
    float64 one rounded to float32 (the device's logf and log10f may differ from it by one and two units in the last
    place: without a log the twin equals the kernel bit for bit)."""
    x, L = _args(x, spec)
    f32 = np.float32
    T = int(spec.frames(L))
    rows = x.reshape(-1, L)
    R, hop, n_bins = rows.shape[0], spec.hop_length, spec.n_bins
    N = spec.lens.astype(np.int64)
    N0, c = int(N[0]), N // 2
    # every bin's kernel on the grid of the longest, centred: G [N0, 2, n_bins]; tap m of the grid is tap m - (c_0 - c_k) of bin k
    G = np.zeros((N0, 2, n_bins), dtype=f32)
    first = c[0] - c
    for k in range(n_bins):
        G[first[k]:first[k] + N[k], 0, k], G[first[k]:first[k] + N[k], 1, k] = spec.kernel(k)
    fr = _taps(rows, T, hop, int(c[0]), N0, f32).reshape(R * T, N0)                 # the span of the longest holds every bin's
    acc = np.zeros((R * T, 2, n_bins), dtype=f32)
    with np.errstate(all="ignore"):
        for m in range(N0):
            on = (first <= m) & (m < first + N)                                       # the bins that have a tap here: no other is touched
            acc[:, :, on] = _fma(G[m][None, :, on], fr[:, m, None, None], acc[:, :, on])
        re, im = acc[:, 0], acc[:, 1]
        v = _fma(re, re, (im * im).astype(f32))
        if spec.power == 1:
            v = np.sqrt(v.astype(np.float64)).astype(f32)     # (the float64 root of a float32, rounded, is the correctly rounded float32 root)
        if spec.log is not None:
            v = np.maximum(v, f32(spec.floor))
            v = (np.log(v.astype(np.float64)) if spec.log == "ln" else np.log10(v.astype(np.float64))).astype(f32)
    return np.ascontiguousarray(v.reshape(R, T, n_bins).transpose(0, 2, 1)).reshape(x.shape[:-1] + (n_bins, T))


# ---- on the device -------------------------------------------------------------------------------------------------------------
def cqt(pcm, spec, lengths=None):
    """Constant-Q features on the GPU: pcm float32 [..., T] on the device (as `load`, `load_batch` and `crops` return it),
    T >= 1, to float32 [..., spec.n_bins, 1 + T // hop]; one kernel, asynchronous on the current stream.  Every row is
    transformed over its whole T (what lies behind a file's or a crop's length is the zeros the decode wrote).  lengths (a
    sequence or an integer tensor): returns (features, lengths // hop + 1 as an int64 tensor where `lengths` was; an entry of
    -1 stays -1)."""
    def short(T):
        if T < 1:
            return f"T = {T} frames: the transform needs a sample"

    return _on_device(pcm, spec, ConstantQ, "[..., T]", short, lengths)
