"""The two normalisations between crops or their log-mel features and a model: mean and variance per line over the frames
that are signal (alacgpu_normalize_meanvar_device) and the clamp relative to the maximum of a clip
(alacgpu_normalize_top_device), csrc/alac_normalize.hip.

The data is float32 [B, ..., n]; a line is the last dimension.

MeanVar(centre, scale, eps), with v = min(max(lengths[b], 0), n) for every line of x[b] (v = n without lengths):

    mean = (sum of x[0 .. v)) / v
    var  = (sum of (x[i] - mean)^2) / v                      two passes, never E[x^2] - mean^2
    y[i] = (x[i] - mean) / sqrt(var + eps)    for i < v      (x[i] - mean with scale off; x[i] / sqrt(var + eps) with centre off)
    y[i] = 0                                  for v <= i < n

v = 0 -- a length of -1, a crop outside the corpus, included -- is a line of zeros.  This is wav2vec 2.0's and HuBERT's
normalisation of a waveform per utterance, and Speech2Text's and Kaldi's CMVN of features per mel bin over the valid frames.

TopDb(top, scale, offset, relative), with mx the maximum of a row, x[b] or with per_channel x[b, c]:

    c = fl(mx - top)
    z = max(x, c)                                   a NaN in either operand gives NaN
    z = fl(z - mx)      only when relative
    y = fl(fl(scale * z) + offset)

Whisper's input is log10 mel power through TopDb.whisper(), (max(x, mx - 8) + 4) / 4; torchaudio's AmplitudeToDB(top_db=80)
on power is TopDb.decibels(80) on log10 power, librosa's power_to_db(ref=np.max, top_db=80) is TopDb.decibels(80, relative=True).

The kernels evaluate both in float32, one IEEE operation at a time, none fused.  For TopDb every operation is exactly rounded
and a maximum has no rounding: the result is specified bit for bit (but for the sign of a zero), and `normalize_host_f32` is
those four lines.  For MeanVar the sums are float32 in a fixed order, which `normalize_host_f32` follows: with P = 64 partial
sums for n <= 256 and P = 1024 above, partial j is ((0 + t[j]) + t[j + P]) + t[j + 2 P] ... in ascending index below v; each
run of 64 partials is added as a tree of halves (q[j] += q[j + h] for h = 32 .. 1), and the 16 sums of those runs by the same
tree (h = 8 .. 1).  Whatever the order, with u = 2^-24, gamma_k = k u / (1 - k u) and d_i = x_i - mean, a float32 evaluation
stays within

    dmean = gamma_{v+1} mean|x|                                        v additions and a division
    dd_i  = (1 + u) dmean + u |d_i|                                    the computed x_i - mean, one rounding
    dV    = (1 + gamma_{v+2}) mean(2 |d_i| dd_i + dd_i^2) + gamma_{v+2} var     a square, v additions and a division
    ds    = dV / (2 s_lo) + 2 u s,   s = sqrt(var + eps),  s_lo = sqrt(max(var - dV, 0) + eps)     the sum and the root
    dY_i  = dd_i / s_lo + |d_i| ds / (s s_lo) + 4 u |y_i|              the numerator, the denominator, the division

of the exact value: |1 / s' - 1 / s| <= ds / (s s_lo) for a computed s' within ds of s that is at least s_lo, and 4 u |y_i|
covers the rounding of the division and its products with the relative errors in front.  With scale off y_i is the computed
d_i: dY_i = dd_i.  With centre off the numerator is x_i itself: dY_i = |x_i| ds / (s s_lo) + 4 u |y_i|.
`normalize_host(..., bound=True)` returns dY.  For TopDb the same call returns what the three roundings can cost,
|scale| u (|c| + |z|) + u |scale z| + u |y|, a bound no correct evaluation uses up.

Input that is not finite follows IEEE arithmetic and is never hidden.  MeanVar: a NaN or an infinity inside 0 .. v reaches
its own line and no other; one at or behind v is never read.  A constant line with eps = 0 is 0 / 0 = NaN.  TopDb: a row with
a NaN anywhere is NaN everywhere (the maximum keeps a NaN, as np.max and torch.amax do) and every other row is untouched;
mx = +inf gives c = +inf, and inf - inf = NaN with relative.

A third kind of `how` is sliding.SlidingMeanVar, Kaldi's sliding-window CMVN (alacgpu_normalize_sliding_device): sliding.py
states it, and `normalize_host`, `normalize_host_f32` and `normalize` take it by handing it on.

A fourth kind is pcen.Pcen, per-channel energy normalisation of mel or constant-Q energies (alacgpu_pcen_device), the one
kind that is a recurrence along time: pcen.py states it, and the same three calls take it by handing it on.

`MeanVar`, `TopDb`, `normalize_host` and `normalize_host_f32` need no device.  `normalize` is the call on device tensors.
"""
import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_device, _lines, _Spec
from .pcen import Pcen, _launch as _pcen_launch, pcen_host, pcen_host_f32
from .sliding import LDS_MAX as _SLIDING_LDS_MAX, RING_WINDOW_MAX as _SLIDING_RING_WINDOW_MAX, SlidingMeanVar, sliding_host, sliding_host_f32

_U = 2.0 ** -24
WAVE_MAX = 256            # ALAC_NORM_WAVE_MAX of csrc/alac_normalize.h: up to here a line has 64 partial sums, above 1024
_LANES, _LINE_THREADS = 64, 1024


class MeanVar(_Spec):
    """Zero mean (centre) and unit variance (scale) per line over its valid elements, zeros behind them; eps is added to the
    variance under the root.  Immutable.  ValueError: eps negative or not finite in float32, centre and scale both off."""

    __slots__ = ("centre", "scale", "eps")

    def __init__(self, centre=True, scale=True, eps=0.0):
        s = object.__setattr__
        if not isinstance(centre, (bool, np.bool_)) or not isinstance(scale, (bool, np.bool_)):
            raise ValueError("centre and scale must be booleans")
        if not centre and not scale:
            raise ValueError("centre and scale are both off: nothing to do")
        s(self, "centre", bool(centre))
        s(self, "scale", bool(scale))
        s(self, "eps", _f32_finite("eps", eps, 0.0))


class TopDb(_Spec):
    """scale * (max(x, mx - top) [- mx with relative]) + offset, mx the maximum of a crop (of each of its channels with
    per_channel).  Immutable.  ValueError: top negative or not finite in float32, scale or offset not finite in float32."""

    __slots__ = ("top", "scale", "offset", "relative", "per_channel")

    def __init__(self, top=8.0, scale=1.0, offset=0.0, relative=False, per_channel=False):
        s = object.__setattr__
        if not isinstance(relative, (bool, np.bool_)) or not isinstance(per_channel, (bool, np.bool_)):
            raise ValueError("relative and per_channel must be booleans")
        s(self, "top", _f32_finite("top", top, 0.0))
        s(self, "scale", _f32_finite("scale", scale))
        s(self, "offset", _f32_finite("offset", offset))
        s(self, "relative", bool(relative))
        s(self, "per_channel", bool(per_channel))

    @classmethod
    def whisper(cls):
        """(max(x, mx - 8) + 4) / 4 on log10 mel power: Whisper's input"""
        return cls(8.0, 0.25, 1.0)

    @classmethod
    def decibels(cls, top_db=80.0, relative=False):
        """Decibels of log10 power, at most top_db below the maximum; relative: with the maximum at 0 dB"""
        return cls(_f32_finite("top_db", top_db, 0.0) / 10.0, 10.0, 0.0, relative)


def _host_args(x, how, lengths):
    """x as [B, lines, n] float32, v [B] int64, and the TopDb rows as [rows, elems per row] shape"""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    if not isinstance(how, (MeanVar, TopDb)):
        raise ValueError(f"how must be a MeanVar or a TopDb, not {how!r}")
    if x.ndim < 2 or (isinstance(how, TopDb) and how.per_channel and x.ndim < 3):
        raise ValueError(f"x must be [B, ..., n]{' with a channel dimension' if x.ndim >= 2 else ''}, not {x.shape}")
    B, n = x.shape[0], x.shape[-1]
    v = np.full(B, n, dtype=np.int64)
    if lengths is not None and isinstance(how, MeanVar):
        lens = np.asarray(lengths)
        if lens.shape != (B,) or (B and lens.dtype.kind not in "iu"):
            raise ValueError(f"lengths must be {B} integers, not {lens.shape} {lens.dtype}")
        v = np.clip(lens.astype(np.int64), 0, n)
    return x, v


def normalize_host(x, how, lengths=None, bound=False):
    """The specification in numpy: x float32 [B, ..., n] to float64 of that shape -- float64 arithmetic on the float32 input
    and the float32 values of `how`'s parameters.  lengths: [B] integers, MeanVar's (ignored by TopDb).  bound=True: returns
    (y, dY), dY float64 like y: how far a float32 evaluation may be from y (the module docstring's chain).  A SlidingMeanVar:
    sliding.sliding_host.  A Pcen: pcen.pcen_host."""
    if isinstance(how, SlidingMeanVar):
        return sliding_host(x, how, lengths, bound)
    if isinstance(how, Pcen):
        return pcen_host(x, how, lengths, bound)
    x, v = _host_args(x, how, lengths)
    shape = x.shape
    B, n = shape[0], shape[-1]
    y = np.zeros(shape, dtype=np.float64)
    dY = np.zeros(shape, dtype=np.float64) if bound else None
    with np.errstate(all="ignore"):
        if isinstance(how, TopDb):
            top, scale, offset = (float(np.float32(a)) for a in (how.top, how.scale, how.offset))
            rows = x.reshape((B * shape[1], -1) if how.per_channel else (B, -1)).astype(np.float64)
            if rows.shape[1]:
                mx = rows.max(axis=1, keepdims=True)             # (np.max keeps a NaN)
                c = mx - top
                z = np.maximum(rows, c)
                if how.relative:
                    z = z - mx
                y = (scale * z + offset).reshape(shape)
                if bound:
                    dY = (abs(scale) * _U * (np.abs(c) + np.abs(z)) + _U * np.abs(scale * z)).reshape(shape) + _U * np.abs(y)
            return (y, dY) if bound else y
        eps = float(np.float32(how.eps))
        for b in range(B):
            k = int(v[b])
            if k == 0:
                continue
            X = x[b].reshape(-1, n)[:, :k].astype(np.float64)
            mean = X.mean(axis=1, keepdims=True)
            d = X - mean
            var = (d * d).mean(axis=1, keepdims=True)
            s = np.sqrt(var + eps)
            out = (d if how.centre else X) / s if how.scale else d
            y[b].reshape(-1, n)[:, :k] = out
            if bound:
                g1, g2 = (k + 1) * _U / (1 - (k + 1) * _U), (k + 2) * _U / (1 - (k + 2) * _U)
                dmean = g1 * np.abs(X).mean(axis=1, keepdims=True)
                dd = (1 + _U) * dmean + _U * np.abs(d)
                if not how.scale:
                    dY[b].reshape(-1, n)[:, :k] = dd
                    continue
                dV = (1 + g2) * (2 * np.abs(d) * dd + dd * dd).mean(axis=1, keepdims=True) + g2 * var
                s_lo = np.sqrt(np.maximum(var - dV, 0.0) + eps)
                ds = dV / (2 * s_lo) + 2 * _U * s
                num = np.abs(d) if how.centre else np.abs(X)
                dY[b].reshape(-1, n)[:, :k] = (dd / s_lo if how.centre else 0.0) + num * ds / (s * s_lo) + 4 * _U * np.abs(out)
    return (y, dY) if bound else y


def _tree_p(t, P):
    """The kernel's float32 sum of t [lines, k] over its last axis with P partial sums (the module docstring's order); returns
    [lines, 1].  Elements added as +0 change nothing, so a line is padded with zeros up to whole rounds of P."""
    f32 = np.float32
    lines, k = t.shape
    rounds = -(-k // P)
    pad = np.zeros((lines, rounds * P), dtype=f32)
    pad[:, :k] = t
    pad = pad.reshape(lines, rounds, P)
    q = np.zeros((lines, P), dtype=f32)
    for r in range(rounds):
        q = (q + pad[:, r, :]).astype(f32)
    q = q.reshape(lines, P // _LANES, _LANES)
    h = _LANES // 2
    while h >= 1:
        q = (q[:, :, :h] + q[:, :, h:2 * h]).astype(f32)
        h //= 2
    w = q[:, :, 0]                                      # [lines, runs of 64]
    h = w.shape[1] // 2
    while h >= 1:
        w = (w[:, :h] + w[:, h:2 * h]).astype(f32)
        h //= 2
    return w[:, :1]


def normalize_host_f32(x, how, lengths=None):
    """The kernel's arithmetic in numpy, one float32 operation at a time: x float32 [B, ..., n] to float32 of that shape.
    MeanVar: the sums in the kernel's documented order (the number of partial sums follows n, as the kernel's mapping does).
    TopDb: the four lines of the module docstring.  Its distance from `normalize_host` is what a correct float32 evaluation
    costs: the tests hold the kernel to a small multiple of that.  A SlidingMeanVar: sliding.sliding_host_f32, the kernel bit
    for bit.  A Pcen: pcen.pcen_host_f32, the kernel bit for bit."""
    if isinstance(how, SlidingMeanVar):
        return sliding_host_f32(x, how, lengths)
    if isinstance(how, Pcen):
        return pcen_host_f32(x, how, lengths)
    x, v = _host_args(x, how, lengths)
    f32 = np.float32
    shape = x.shape
    B, n = shape[0], shape[-1]
    y = np.zeros(shape, dtype=f32)
    with np.errstate(all="ignore"):
        if isinstance(how, TopDb):
            top, scale, offset = f32(how.top), f32(how.scale), f32(how.offset)
            rows = x.reshape((B * shape[1], -1) if how.per_channel else (B, -1))
            if rows.shape[1]:
                mx = rows.max(axis=1, keepdims=True)
                c = (mx - top).astype(f32)
                z = np.maximum(rows, c)
                if how.relative:
                    z = (z - mx).astype(f32)
                y = ((scale * z).astype(f32) + offset).astype(f32).reshape(shape)
            return y
        eps = f32(how.eps)
        P = _LANES if n <= WAVE_MAX else _LINE_THREADS
        for b in range(B):
            k = int(v[b])
            if k == 0:
                continue
            X = x[b].reshape(-1, n)[:, :k]
            fv = f32(k)
            mean = (_tree_p(X, P) / fv).astype(f32)
            d = (X - mean).astype(f32)
            if how.scale:
                var = (_tree_p((d * d).astype(f32), P) / fv).astype(f32)
                s = np.sqrt((var + eps).astype(f32)).astype(f32)
                out = ((d if how.centre else X) / s).astype(f32)
            else:
                out = d
            y[b].reshape(-1, n)[:, :k] = out
    return y


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _normalize(ctx, x, how, lengths, out):
    """`normalize`; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`), asked for behind the checks"""
    import torch

    if not isinstance(how, (MeanVar, TopDb, SlidingMeanVar, Pcen)):
        raise ValueError(f"how must be a MeanVar, a TopDb, a SlidingMeanVar or a Pcen, not {how!r}")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError("x must be a float32 device tensor [B, ..., n]")
    top = isinstance(how, TopDb)
    if top and how.per_channel and x.dim() < 3:
        raise ValueError("per_channel needs x [B, C, ..., n]")
    pcen = isinstance(how, Pcen)
    if pcen and how.lines is not None and (x.dim() != 4 or x.shape[2] != how.lines):
        raise ValueError(f"a Pcen with {how.lines} values per parameter needs x [B, C, {how.lines}, n], not {tuple(x.shape)}")
    layout = _lines(x) if x.numel() else (max(x.shape[-1], 1), x.shape[-1])
    if layout is None:
        raise ValueError("x must be contiguous or the slice [..., :n] of a contiguous tensor")
    S, n = layout
    sliding = isinstance(how, SlidingMeanVar)
    if sliding and n > _SLIDING_LDS_MAX and how.window > _SLIDING_RING_WINDOW_MAX:
        raise ValueError(f"lines of {n} frames: above {_SLIDING_LDS_MAX} a sliding window takes at most {_SLIDING_RING_WINDOW_MAX} frames")
    if out is None:
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    elif (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
          or (x.numel() and _lines(out) != layout)):
        raise ValueError("out must be x itself or a float32 tensor of x's shape, layout and device")
    B = x.shape[0]
    d_valid = None if top else _lengths_device("lengths", lengths, B, x.device)
    if x.numel() == 0:
        return out
    rows = B * x.shape[1] if top and how.per_channel else B
    lines_per_row = x.numel() // n // rows
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if pcen:
            _pcen_launch(ctx(), x, out, rows, lines_per_row, S, n, d_valid, how, stream)
        elif sliding:
            ctx().normalize_sliding_device(x, out, rows, lines_per_row, S, n, d_valid, how.window, how.min_window, how.center,
                                           how.norm_vars, stream=stream)
        elif top:
            ctx().normalize_top_device(x, out, rows, lines_per_row, S, n, how.top, how.scale, how.offset, how.relative, stream=stream)
        else:
            ctx().normalize_meanvar_device(x, out, rows, lines_per_row, S, n, d_valid, how.centre, how.scale, how.eps, stream=stream)
    return out


def normalize(x, how, lengths=None, out=None):
    """Normalise on the GPU: x float32 [B, ..., n] on the device, contiguous or the slice [..., :n] of a contiguous tensor
    (Whisper drops the last frame: normalize(feats[..., :-1], TopDb.whisper())); what lies behind the slice is neither read
    nor written.  how: a `MeanVar` -- every line x[b, ..., :] over its first lengths[b] elements, zeros behind them --, a
    `TopDb` -- every row x[b], or x[b, c] with per_channel, against its own maximum -- or a sliding.SlidingMeanVar -- every frame
    of a line against the window around or behind it, zeros behind lengths[b] -- or a pcen.Pcen -- per-channel energy
    normalisation of every line of energies, zeros behind lengths[b]; one with per-bin sequences needs x [B, C, L, n].  lengths: [B] integers, a sequence or a
    tensor (as `crops` returns them; -1 counts as 0, more than n as n), not used by TopDb; default: whole lines.  out: x
    itself (in place) or a tensor of x's shape and layout; default: a new one of x's layout.  Returns out.  One launch
    (MeanVar, SlidingMeanVar, Pcen) or two (TopDb), asynchronous on the current stream; ValueError before any device work."""
    ctx = _device_context("x", x, "[B, ..., n]")
    if not isinstance(how, (MeanVar, TopDb, SlidingMeanVar, Pcen)):
        raise ValueError(f"how must be a MeanVar, a TopDb, a SlidingMeanVar or a Pcen, not {how!r}")
    return _normalize(ctx, x, how, lengths, out)
