"""The energy VAD of the Kaldi speaker recipes and the selection of the voiced frames behind the features:
`compute-vad-decision` (alacgpu_vad_energy_device) and `select-voiced-frames` (alacgpu_select_frames_device), one launch each,
csrc/alac_vad.hip.  Neither Kaldi nor torchaudio is at hand where this is built: the parity is with this written
specification, Kaldi's `ComputeVadEnergy` restated, not with foreign fixtures.

The features are float32 [B, C, lines, n] (or [B, lines, n]); E[t] is feature `line` of row b's first channel -- c0 or the log
energy of raw MFCCs --, v = min(max(lengths[b], 0), n) its valid frames (n without lengths).  EnergyVad(energy_threshold,
energy_mean_scale, frames_context = c, proportion_threshold, line):

    thr     = energy_threshold + energy_mean_scale * (sum of E[0 .. v)) / v          (thr = energy_threshold when the scale is 0)
    num[t]  = #{t2 in [t - c, t + c] and [0, v) : E[t2] > thr},   den[t] = #{t2 in [t - c, t + c] and [0, v)}
    mask[t] = 1 if num[t] >= den[t] * proportion_threshold else 0;   0 for t >= v

`vad_host` is this with the threshold in float64.  In float32 (`vad_host_f32`, the kernel bit for bit): the sum in `MeanVar`'s order
(normalize._tree_p: 64 partial sums for n <= 256, 1024 above), mean = fl(sum / fl(v)), thr = fl(energy_threshold +
fl(scale * mean)), nothing contracted, the division correctly rounded; the counts are integers, and the last comparison is
float32(num) >= fl(float32(den) * proportion_threshold).  A NaN energy compares false, and a NaN anywhere below v makes thr
NaN unless the scale is 0: then nothing is above it.  With a scale of 0 the mean is not computed.

The only rounding that can change a decision is the threshold's.  With u = 2^-24 and gamma_k = k u / (1 - k u) the float32
thr is within

    dthr = |scale| (gamma_{v+1} mean|E| + u |mean|) (1 + u) + u |thr|        the mean (v additions, a division), the product, the sum

of the exact one, whatever the order of the sum: a frame with |E[t] - thr| > dthr counts the same in any correct float32
evaluation.  `vad_host(..., margin=True)` returns |E[t] - thr| per frame and dthr per row.  The last comparison is Kaldi's own,
an integer count against one float32 product, exactly specified: `vad_host` makes it in float32 too (in float64
5 * float32(0.6) is above 3, in float32 it rounds to 3).

`select_host(x, mask, lengths)`: for every line of row b, y[k] = x[t_k] with t_k the k-th t < v whose mask[b, t] != 0, zeros
from the voiced count up to n; new_lengths[b] is the voiced count, or lengths[b] itself where that is negative (a crop
outside the corpus stays one).  It moves bits only: it is its own float32 twin.

`EnergyVad`, `vad_host`, `vad_host_f32` and `select_host` need no device.  `vad_energy` and `select_frames` are the calls on
device tensors.
"""
import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_device, _lengths_host, _lines, _Spec

_U = 2.0 ** -24
MAX_CONTEXT = 64                  # ALAC_VAD_MAX_CONTEXT of csrc/alac_vad.h
WAVE_MAX = 256                    # ALAC_VAD_WAVE_MAX: up to here the mean has 64 partial sums, above 1024 (normalize.WAVE_MAX)


class EnergyVad(_Spec):
    """Kaldi's energy VAD (VadEnergyOptions, its defaults) on feature `line` of the first channel: a frame is voiced when at
    least proportion_threshold of the frames within frames_context of it have an energy above energy_threshold +
    energy_mean_scale * the mean energy.  Immutable.  ValueError: a threshold or the scale not finite in float32,
    energy_mean_scale < 0, frames_context outside 0 .. 64, proportion_threshold outside 0 .. 1, line negative."""

    __slots__ = ("energy_threshold", "energy_mean_scale", "frames_context", "proportion_threshold", "line")

    def __init__(self, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6, line=0):
        s = object.__setattr__
        s(self, "energy_threshold", _f32_finite("energy_threshold", energy_threshold))
        s(self, "energy_mean_scale", _f32_finite("energy_mean_scale", energy_mean_scale, 0.0))
        for name, v, most in (("frames_context", frames_context, MAX_CONTEXT), ("line", line, (1 << 31) - 1)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= most:
                raise ValueError(f"{name} must be an integer of 0 .. {most}, not {v!r}")
            s(self, name, int(v))
        p = _f32_finite("proportion_threshold", proportion_threshold, 0.0)
        if p > 1.0:
            raise ValueError(f"proportion_threshold must be in 0 .. 1, not {proportion_threshold!r}")
        s(self, "proportion_threshold", p)

    @classmethod
    def voxceleb(cls):
        """--vad-energy-threshold=5.5 --vad-energy-mean-scale=0.5 --vad-frames-context=2 --vad-proportion-threshold=0.12: the
        conf/vad.conf of Kaldi's VoxCeleb and SRE recipes"""
        return cls(5.5, 0.5, 2, 0.12)


def _host_args(x, vad, lengths):
    """The energies [B, n] float32 of x [B, C, lines, n] or [B, lines, n], and v [B]"""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim not in (3, 4):
        raise ValueError(f"x must be float32 [B, C, lines, n] or [B, lines, n], not {x.dtype} {x.shape}")
    if not isinstance(vad, EnergyVad):
        raise ValueError(f"vad must be an EnergyVad, not {vad!r}")
    if vad.line >= x.shape[-2] or (x.ndim == 4 and x.shape[0] and x.shape[1] == 0):
        raise ValueError(f"line {vad.line} of features with {x.shape[-2]} lines")
    E = x[:, 0, vad.line, :] if x.ndim == 4 else x[:, vad.line, :]
    return E, _lengths_host("lengths", lengths, x.shape[0], x.shape[-1])


def _decide(over, v, c, proportion):
    """mask [v] uint8 from over [v] bool: the counts over t - c .. t + c inside 0 .. v and the last comparison, in float32"""
    t = np.arange(v)
    lo, hi = np.maximum(t - c, 0), np.minimum(t + c, v - 1) + 1
    cum = np.concatenate([[0], np.cumsum(over.astype(np.int64))])
    num, den = cum[hi] - cum[lo], hi - lo
    return (num.astype(np.float32) >= (den.astype(np.float32) * np.float32(proportion)).astype(np.float32)).astype(np.uint8)


def vad_host(x, vad, lengths=None, margin=False):
    """The specification in numpy: the decisions uint8 [B, n] from x float32 [B, C, lines, n] or [B, lines, n], float64
    arithmetic on the float32 input and the float32 values of `vad`'s parameters.  lengths: [B] integers (below 0 counts as
    0, above n as n); default: n.  margin=True: returns (mask, |E[t] - thr| float64 [B, n] -- infinite at and behind v --,
    dthr float64 [B]): a frame whose distance is above its row's dthr is on the same side of any correct float32 threshold."""
    E, lens = _host_args(x, vad, lengths)
    B, n = E.shape
    mask = np.zeros((B, n), dtype=np.uint8)
    dist = np.full((B, n), np.inf)
    dthr = np.zeros(B)
    thr0, scale = float(np.float32(vad.energy_threshold)), float(np.float32(vad.energy_mean_scale))
    with np.errstate(all="ignore"):
        for b in range(B):
            v = int(lens[b])
            if v == 0:
                continue
            e = E[b, :v].astype(np.float64)
            mean = e.mean() if scale != 0.0 else 0.0
            thr = thr0 + scale * mean
            mask[b, :v] = _decide(e > thr, v, vad.frames_context, vad.proportion_threshold)
            dist[b, :v] = np.abs(e - thr)
            g = (v + 1) * _U / (1 - (v + 1) * _U)
            dthr[b] = scale * (g * np.abs(e).mean() + _U * abs(mean)) * (1 + _U) + _U * abs(thr) if scale != 0.0 else 0.0
    return (mask, dist, dthr) if margin else mask


def vad_host_f32(x, vad, lengths=None):
    """The kernel's arithmetic in numpy, bit for bit: the decisions uint8 [B, n], the threshold one float32 operation at a
    time with the sum in the kernel's order"""
    from .normalize import _LANES, _LINE_THREADS, _tree_p

    E, lens = _host_args(x, vad, lengths)
    f32 = np.float32
    B, n = E.shape
    mask = np.zeros((B, n), dtype=np.uint8)
    thr0, scale = f32(vad.energy_threshold), f32(vad.energy_mean_scale)
    with np.errstate(all="ignore"):
        for b in range(B):
            v = int(lens[b])
            if v == 0:
                continue
            e = E[b, :v]
            thr = thr0
            if scale != 0.0:
                mean = (_tree_p(e[None, :], _LANES if n <= WAVE_MAX else _LINE_THREADS)[0, 0] / f32(v)).astype(f32)
                thr = f32(thr0 + f32(scale * mean))
            mask[b, :v] = _decide(e > thr, v, vad.frames_context, vad.proportion_threshold)
    return mask


def select_host(x, mask, lengths=None):
    """`select-voiced-frames` in numpy: x [B, ..., n] (any dtype) and mask [B, n] to (y like x, new_lengths int64 [B]): every
    line of row b keeps its frames t < v with mask[b, t] != 0, in order, zeros behind them; new_lengths[b] their number, or
    lengths[b] where that is negative"""
    x, mask = np.asarray(x), np.asarray(mask)
    if x.ndim < 2 or mask.shape != (x.shape[0], x.shape[-1]):
        raise ValueError(f"x must be [B, ..., n] and mask [B, n], not {x.shape} and {mask.shape}")
    B, n = x.shape[0], x.shape[-1]
    lens = _lengths_host("lengths", lengths, B, n)
    new = np.zeros(B, dtype=np.int64)
    y = np.zeros_like(x)
    for b in range(B):
        keep = np.nonzero(mask[b, :int(lens[b])] != 0)[0]
        y[b].reshape(-1, n)[:, :len(keep)] = x[b].reshape(-1, n)[:, keep]
        new[b] = len(keep)
    if lengths is not None:
        given = np.asarray(lengths).astype(np.int64)
        new = np.where(given < 0, given, new)
    return y, new


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _features_layout(name, x):
    """(B, lines per row, feature lines, line stride, n) of x, a float32 device tensor [B, C, lines, n] or [B, lines, n],
    contiguous or the slice [..., :n] of a contiguous tensor; ValueError otherwise"""
    import torch

    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() not in (3, 4):
        raise ValueError(f"{name} must be a float32 device tensor [B, C, lines, n] or [B, lines, n]")
    layout = _lines(x) if x.numel() else (max(x.shape[-1], 1), x.shape[-1])
    if layout is None:
        raise ValueError(f"{name} must be contiguous or the slice [..., :n] of a contiguous tensor")
    per_row = x.shape[1] * x.shape[2] if x.dim() == 4 else x.shape[1]
    return x.shape[0], per_row, x.shape[-2], layout[0], layout[1]


def _vad_energy(ctx, feats, vad, lengths, out=None):
    """`vad_energy` behind its first check; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`); out:
    a contiguous uint8 tensor [B, n] to write (the corpus's scratch)"""
    import torch

    if not isinstance(vad, EnergyVad):
        raise ValueError(f"vad must be an EnergyVad, not {vad!r}")
    B, per_row, lines, S, n = _features_layout("feats", feats)
    if vad.line >= lines:
        raise ValueError(f"line {vad.line} of features with {lines} lines")
    d_valid = _lengths_device("feat_lengths", lengths, B, feats.device)
    mask = torch.empty((B, n), dtype=torch.uint8, device=feats.device) if out is None else out
    if feats.numel() == 0:
        return mask
    with torch.cuda.device(feats.device):
        stream = torch.cuda.current_stream(feats.device).cuda_stream
        ctx().vad_energy_device(feats, B, per_row * S, vad.line * S, n, d_valid, vad.energy_threshold, vad.energy_mean_scale,
                                vad.frames_context, vad.proportion_threshold, mask, n, stream=stream)
    return mask


def vad_energy(feats, vad, feat_lengths=None):
    """The energy VAD on the GPU: feats float32 [B, C, lines, n] or [B, lines, n] on the device, contiguous or the slice
    [..., :n] of a contiguous tensor; vad: an `EnergyVad`; feat_lengths: [B] integers, a sequence or a tensor (as `crops`
    returns them; -1 counts as 0, more than n as n); default: n.  Returns the decisions, uint8 [B, n]: 1 where frame t of row
    b is voiced, 0 where it is not and at and behind the row's length (see the module).  One launch, asynchronous on the
    current stream, nothing is read back; ValueError before any device work."""
    ctx = _device_context("feats", feats, "[B, C, lines, n]")
    return _vad_energy(ctx, feats, vad, feat_lengths)


def _select_frames(ctx, feats, mask, lengths, out, new_lengths=None):
    """`select_frames` behind its first check; ctx() gives the context that runs it"""
    import torch

    B, per_row, _, S, n = _features_layout("feats", feats)
    if (not isinstance(mask, torch.Tensor) or mask.device != feats.device or mask.dtype not in (torch.uint8, torch.bool)
            or mask.shape != (B, n) or (mask.numel() and mask.stride(-1) != 1 and n != 1)):
        raise ValueError(f"mask must be a uint8 or bool tensor [{B}, {n}] on {feats.device} with its frames next to one another")
    if out is None:
        out = torch.empty_strided(feats.shape, feats.stride(), dtype=feats.dtype, device=feats.device)
    elif (not isinstance(out, torch.Tensor) or out.shape != feats.shape or out.dtype != feats.dtype or out.device != feats.device
          or (feats.numel() and _lines(out) != (S, n))):
        raise ValueError("out must be feats itself or a float32 tensor of its shape, layout and device")
    d_valid = _lengths_device("feat_lengths", lengths, B, feats.device)
    if new_lengths is None:
        new_lengths = torch.empty(B, dtype=torch.int64, device=feats.device)
    if feats.numel() == 0:
        return out, (new_lengths.zero_() if d_valid is None else new_lengths.copy_(d_valid.clamp(max=0)))
    mask_stride = mask.stride(0) if B > 1 else n
    if mask_stride < n:
        raise ValueError("the rows of mask overlap")
    with torch.cuda.device(feats.device):
        stream = torch.cuda.current_stream(feats.device).cuda_stream
        ctx().select_frames_device(feats, out, B, per_row, S, n, d_valid, mask.view(torch.uint8) if mask.dtype == torch.bool else mask,
                                   mask_stride, new_lengths, stream=stream)
    return out, new_lengths


def select_frames(feats, mask, feat_lengths=None, out=None):
    """Keep the voiced frames on the GPU: feats float32 [B, C, lines, n] or [B, lines, n] on the device, contiguous or the
    slice [..., :n] of a contiguous tensor; mask: uint8 or bool [B, n] on that device (what `vad_energy` returned);
    feat_lengths as there.  Every line of row b keeps its frames t below the row's length with mask[b, t] != 0, in order, and
    is zero behind them up to n.  out: feats itself (in place: a frame only moves left) or a tensor of its shape and layout;
    default: a new one.  Returns (out, new_lengths): int64 [B] on the device, the voiced counts, feat_lengths[b] itself where
    that is negative.  One launch, asynchronous on the current stream, nothing is read back; ValueError before any device
    work."""
    ctx = _device_context("feats", feats, "[B, C, lines, n]")
    return _select_frames(ctx, feats, mask, feat_lengths, out)
