"""Delta features behind the features: Kaldi's `add-deltas` in one launch (alacgpu_deltas_device, csrc/alac_deltas.hip).  The
features and their time derivatives up to `order`, stacked along the feature axis: x float32 [B, C, F, T] to
[B, C, (order + 1) * F, T], block k = lines k F .. (k + 1) F the order-k deltas, block 0 the features themselves.  Kaldi's
`DeltaFeatures` is the specification, not torchaudio's `compute_deltas`:

    scales_0 = [1];  scales_k = scales_{k-1} convolved with [-W .. W] / (2 * sum of j^2, j = 1 .. W)        (length 2 k W + 1)
    out[k F + f, t] = sum over j = -k W .. k W of scales_k[j + k W] * x[f, clamp(t + j, 0, len - 1)]

with W = window.  The clamp is into the ORIGINAL features for every order: at the edges that is not what two replicate-padded
first-order passes give (those clamp the first pass's output), and the difference is the size of the signal's slope.  The
scales are built in float64 and rounded to float32 once.

len is the row's entry of `lengths`, clamped into 0 .. T (T without lengths).  A frame at or behind len -- every frame of a
row with len <= 0, such as a crop outside the corpus -- gets its static block copied and zeros in every delta block: padding
never leaks into signal (nothing at or behind len is read for a delta) and stays zero behind a `MeanVar`.

The kernel's float32 order: one chain of fused multiply-adds in ascending j from -k W, from zero.  There is no transcendental
in it, so `deltas_host_f32` is the kernel bit for bit, and `deltas_host` (float64 on the float32 scales) is within
(2 k W + 2) u sum over j of |scales_k[j] x[...]|, u = 2^-24, of both.

order is 1 .. 3 and window 1 .. 4: the widest filter has 25 taps.

`delta_scales`, `Deltas`, `deltas_host` and `deltas_host_f32` need no device.  `add_deltas` is the call on device tensors.
"""
import numpy as np

from ._stageargs import _device_context, _fma32, _lengths_device, _lengths_host, _lines, _Spec

MAX_ORDER, MAX_WINDOW = 3, 4


def _order_window(order, window):
    for name, v, most in (("order", order, MAX_ORDER), ("window", window, MAX_WINDOW)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= most:
            raise ValueError(f"{name} must be an integer of 1 .. {most}, not {v!r}")
    return int(order), int(window)


def delta_scales(order, window):
    """Kaldi's delta filters: a tuple of `order` float32 arrays, the k-th (k = 1 .. order) of length 2 k window + 1, computed
    in float64 and rounded once: scales_k = scales_{k-1} convolved with [-window .. window] / (2 sum of j^2), scales_0 = [1]"""
    order, W = _order_window(order, window)
    j = np.arange(-W, W + 1, dtype=np.float64)
    first = j / (2.0 * float((np.arange(1, W + 1) ** 2).sum()))
    out, cur = [], np.ones(1)
    for _ in range(order):
        cur = np.convolve(cur, first)
        out.append(cur.astype(np.float32))
    return tuple(out)


class Deltas(_Spec):
    """Kaldi's add-deltas: the derivatives up to `order` (1 .. 3) over `window` (1 .. 4) frames on each side per order; `scales`
    is `delta_scales(order, window)` as one read-only float32 array, order 1's first (the table alacgpu_deltas_device takes).
    Immutable."""

    __slots__ = ("order", "window")

    def __init__(self, order=2, window=2):
        order, window = _order_window(order, window)
        object.__setattr__(self, "order", order)
        object.__setattr__(self, "window", window)

    @property
    def scales(self):
        table = np.concatenate(delta_scales(self.order, self.window))
        table.flags.writeable = False
        return table

    def lines(self, n):
        """The feature lines behind the stage for n in front of it: (order + 1) * n"""
        return (self.order + 1) * n

    def device_scales(self, device):
        """`scales` on the device (a torch.device), uploaded once per specification and device"""
        import torch

        index = device.index if device.index is not None else torch.cuda.current_device()
        key = (self.order, self.window, index)
        if key not in _DEVICE_SCALES:
            _DEVICE_SCALES[key] = torch.from_numpy(np.array(self.scales)).to(torch.device("cuda", index))
        return _DEVICE_SCALES[key]


_DEVICE_SCALES = {}


def _host_args(x, spec, lengths):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 4:
        raise ValueError(f"x must be float32 [B, C, F, T], not {x.dtype} {x.shape}")
    if not isinstance(spec, Deltas):
        raise ValueError("spec must be a Deltas")
    B, T = x.shape[0], x.shape[3]
    return x, _lengths_host("lengths", lengths, B, T)


def _taps(x_row, length, half):
    """x_row [C, F, T] gathered for a filter of 2 half + 1 taps: [C, F, length, 2 half + 1], tap j of frame t the frame
    clamp(t + j - half, 0, length - 1)"""
    idx = np.clip(np.arange(length)[:, None] + np.arange(-half, half + 1)[None, :], 0, length - 1)
    return x_row[:, :, idx]


def deltas_host(x, spec, lengths=None, bound=False):
    """The kernel's specification in numpy: x float32 [B, C, F, T] to float64 [B, C, (order + 1) F, T] -- float64 arithmetic
    on the float32 input and the float32 scales.  lengths: None or B integers (below 0 counts as 0, above T as T).  bound=True:
    returns (out, d), d float64 like out: (2 k W + 2) u sum over j of |scales_k[j] x[...]| in block k, 0 in block 0 and behind
    the lengths -- how far a float32 chain may be from out."""
    x, lens = _host_args(x, spec, lengths)
    B, C, F, T = x.shape
    out = np.zeros((B, C, (spec.order + 1) * F, T), dtype=np.float64)
    d = np.zeros_like(out)
    out[:, :, :F, :] = x
    for b in range(B):
        n = int(lens[b])
        if n <= 0:
            continue
        for k, sc in enumerate(delta_scales(spec.order, spec.window), start=1):
            g = _taps(x[b].astype(np.float64), n, k * spec.window) * sc.astype(np.float64)
            out[b, :, k * F:(k + 1) * F, :n] = g.sum(axis=-1)
            d[b, :, k * F:(k + 1) * F, :n] = (2 * k * spec.window + 2) * 2.0 ** -24 * np.abs(g).sum(axis=-1)
    return (out, d) if bound else out


def deltas_host_f32(x, spec, lengths=None):
    """The kernel's arithmetic in numpy, bit for bit: x float32 [B, C, F, T] to float32 [B, C, (order + 1) F, T], every delta
    one chain of float32 fused multiply-adds in ascending j from zero"""
    x, lens = _host_args(x, spec, lengths)
    B, C, F, T = x.shape
    out = np.zeros((B, C, (spec.order + 1) * F, T), dtype=np.float32)
    out[:, :, :F, :] = x
    for b in range(B):
        n = int(lens[b])
        if n <= 0:
            continue
        for k, sc in enumerate(delta_scales(spec.order, spec.window), start=1):
            g = _taps(x[b], n, k * spec.window)
            acc = np.zeros(g.shape[:-1], dtype=np.float32)
            for j in range(sc.shape[0]):
                acc = _fma32(sc[j], g[..., j], acc)
            out[b, :, k * F:(k + 1) * F, :n] = acc
    return out


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _add_deltas(ctx, feats, spec, lengths, out):
    """`add_deltas` behind its first check; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`),
    asked for behind the checks"""
    import torch

    if not isinstance(spec, Deltas):
        raise ValueError("spec must be a Deltas")
    if not isinstance(feats, torch.Tensor) or feats.device.type != "cuda" or feats.dtype != torch.float32 or feats.dim() != 4:
        raise ValueError("feats must be a float32 device tensor [B, C, F, T]")
    layout = _lines(feats) if feats.numel() else (max(feats.shape[-1], 1), feats.shape[-1])
    if layout is None:
        raise ValueError("feats must be contiguous or the slice [..., :T] of a contiguous tensor")
    S, T = layout
    B, C, F = feats.shape[:3]
    shape = (B, C, spec.lines(F), T)
    if out is not None and (not isinstance(out, torch.Tensor) or out.shape != shape or out.dtype != torch.float32
                            or out.device != feats.device or (out.numel() and _lines(out) is None)):
        raise ValueError(f"out must be a float32 tensor {shape} on {feats.device}, contiguous or the slice [..., :T] of a contiguous "
                         f"tensor")
    d_lengths = _lengths_device("lengths", lengths, B, feats.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=feats.device)
    if feats.numel() == 0:
        return out
    So = _lines(out)[0]
    a0, a1 = feats.data_ptr(), feats.data_ptr() + 4 * ((B * C * F - 1) * S + T)
    o0, o1 = out.data_ptr(), out.data_ptr() + 4 * ((B * C * shape[2] - 1) * So + T)
    if a0 < o1 and o0 < a1:
        raise ValueError("out overlaps feats")
    with torch.cuda.device(feats.device):
        stream = torch.cuda.current_stream(feats.device).cuda_stream
        ctx().deltas_device(feats, out, B, C, F, S, So, T, d_lengths, spec.order, spec.window, spec.device_scales(feats.device),
                            stream=stream)
    return out


def add_deltas(feats, spec, lengths=None, out=None):
    """Delta features on the GPU: feats float32 [B, C, F, T] on the device, contiguous or the slice [..., :T] of a contiguous
    tensor, to float32 [B, C, (spec.order + 1) * F, T]: the features, then their deltas of order 1 .. spec.order (see the
    module).  lengths: [B] integers, a sequence or a tensor (the feat_lengths `crops` returns; -1 counts as 0, more than T as
    T): the frames of a row that are signal; a frame behind them keeps its features and gets zero deltas; default: T.  out: a
    float32 tensor of the result's shape apart from feats (never in place: the shape grows); default: a new one.  Returns
    out.  One launch, asynchronous on the current stream; ValueError before any device work for anything else."""
    ctx = _device_context("feats", feats, "[B, C, F, T]")
    return _add_deltas(ctx, feats, spec, lengths, out)
