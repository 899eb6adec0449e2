"""What the stage calls behind the crops -- `reverb`, `mix`, `log_mel`, `normalize`, `spec_augment` -- share in front of their one library
call: the immutable specification base (`_Spec`, `_f32_finite`), the lengths on both sides (`_lengths_host`,
`_lengths_device`), the layouts a kernel takes (`_lines`, `_planes`, `_span`), the context of a tensor's device
(`_device_context`), the tree of halves and the exact fused multiply-add of the float32 twins (`_tree`, `_fma32`), and `_signal_and_companion`: the one check of a
float32 signal [B, C, T] with a companion [B, C or 1, T'], two optional lengths and an `out`, which is all of `_mix` and
`_reverb` but their library call.  A new stage takes what its tensor function needs from here, never from another stage's
module; what its keyword of `Corpus.crops` refuses and draws goes into `_cropstages.py`, what it runs into `Corpus._run`.
"""
import math

import numpy as np

_F32_OVERFLOW = float(2 ** 128 - 2 ** 103)      # what rounds to infinity in float32, and above


def _f32_finite(name, v, least=None):
    """v as a float that is finite in float32 (and at least `least`); ValueError otherwise"""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, not {v!r}")
    v = float(v)
    if not math.isfinite(v) or abs(v) >= _F32_OVERFLOW or (least is not None and v < least):
        raise ValueError(f"{name} must be finite in float32{'' if least is None else f' and at least {least}'}, not {v!r}")
    return v


class _Spec:
    __slots__ = ()

    def __setattr__(self, name, value):
        raise AttributeError(f"a {type(self).__name__} is immutable")

    def __delattr__(self, name):
        raise AttributeError(f"a {type(self).__name__} is immutable")

    def __eq__(self, other):
        return type(other) is type(self) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash((type(self).__name__,) + tuple(getattr(self, k) for k in self.__slots__))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={getattr(self, k)!r}' for k in self.__slots__)})"


def _tree(q):
    """q [..., 2^k] float32 added over its last axis as a tree of halves: q[j] += q[j + h] for h = 2^(k-1) .. 1"""
    h = q.shape[-1] // 2
    while h >= 1:
        q = (q[..., :h] + q[..., h:2 * h]).astype(np.float32)
        h //= 2
    return q[..., 0]


def _fma32(x, y, z):
    """fma(x, y, z) of float32 arrays, exactly: the product is exact in float64, the sum is rounded to odd there (TwoSum tells
    which way the exact sum lies), and 53 bits rounded to odd round to float32 as the exact value does"""
    p = np.asarray(x, dtype=np.float32).astype(np.float64) * np.asarray(y, dtype=np.float32).astype(np.float64)
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    p, z = np.broadcast_arrays(p, z)
    s = p + z
    t = s - p
    err = (p - (s - t)) + (z - t)
    bits = np.ascontiguousarray(s).view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    bits = np.where(fix, bits + np.where((err > 0) == (s > 0), 1, -1), bits)
    return bits.view(np.float64).astype(np.float32)


def _lengths_host(name, lengths, B, T):
    """lengths as int64 [B] clamped into 0 .. T (T for every row without them), for the specifications in numpy"""
    if lengths is None:
        return np.full(B, T, dtype=np.int64)
    lens = np.asarray(lengths)
    if lens.shape != (B,) or (B and lens.dtype.kind not in "iu"):
        raise ValueError(f"{name} must be {B} integers, not {lens.shape} {lens.dtype}")
    return np.clip(lens.astype(np.int64), 0, T)


def _lengths_device(name, lengths, B, device):
    """lengths (None, a sequence or a tensor of B integers) as a contiguous int64 tensor on `device`, or None"""
    import torch

    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype.is_floating_point or lengths.dtype == torch.bool or lengths.shape != (B,):
            raise ValueError(f"{name} must be {B} integers")
        return lengths.to(device, torch.int64).contiguous()
    lens = np.asarray(lengths)
    if lens.shape != (B,) or (B and lens.dtype.kind not in "iu"):
        raise ValueError(f"{name} must be {B} integers")
    return torch.from_numpy(lens.astype(np.int64)).to(device)


def _lines(x):
    """(line_stride, n) of x [B, ..., n]: x is contiguous (line_stride = n) or the slice [..., :n] of a contiguous tensor
    whose last dimension is line_stride; None for any other view"""
    n = x.shape[-1]
    if n != 1 and x.stride(-1) != 1:
        return None
    S, expect = None, None
    for k in range(x.dim() - 2, -1, -1):
        if x.shape[k] == 1:
            continue
        if S is None:
            S = x.stride(k)
            if S < n:
                return None
            expect = S * x.shape[k]
        else:
            if x.stride(k) != expect:
                return None
            expect *= x.shape[k]
    return (n if S is None else S), n


def _planes(name, t, B=None, T=None, channels=None):
    """The plane stride of t, a float32 device tensor [B, C, T], contiguous or the slice [..., :T] of a contiguous one"""
    import torch

    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 3 or t.shape[1] == 0:
        raise ValueError(f"{name} must be a float32 device tensor [B, C, T]")
    if (B is not None and t.shape[0] != B) or (T is not None and t.shape[2] != T) or (channels is not None and t.shape[1] not in channels):
        raise ValueError(f"{name} must be [{B}, {' or '.join(str(c) for c in channels)}, {T}], not {tuple(t.shape)}")
    layout = _lines(t) if t.numel() else (max(t.shape[-1], 1), t.shape[-1])
    if layout is None:
        raise ValueError(f"{name} must be contiguous or the slice [..., :T] of a contiguous tensor")
    return layout[0]


def _span(t, stride):
    """The addresses [first, behind the last) of the elements of t [B, C, T] with that plane stride"""
    B, C, T = t.shape
    return t.data_ptr(), t.data_ptr() + 4 * ((B * C - 1) * stride + T)


def _device_context(name, x, shape):
    """The first step of every public stage call: x is a device tensor (ValueError naming it and `shape` otherwise); returns
    the function that gives the context of its device, asked for behind the other checks"""
    import torch

    from .resample import _context

    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise ValueError(f"{name} must be a float32 device tensor {shape}")
    index = x.device.index if x.device.index is not None else torch.cuda.current_device()
    return lambda: _context(index)


def _signal_and_companion(x, name, other, lengths, other_lengths, out, same_frames):
    """The arguments of a stage that changes a signal by a companion per row: x float32 [B, C, T] and `other` (called `name`
    in the messages) float32 [B, C or 1, T'] on x's device, each contiguous or the slice [..., :T] of a contiguous tensor;
    T' == T with same_frames, else T' = K >= 1 of its own; lengths and `name`_lengths None or B integers (a sequence or a
    tensor); out None, x itself, or a tensor of x's shape and layout that overlaps neither.  ValueError otherwise, before
    any device work.  Returns (x's plane stride, other's, out -- a new tensor of x's layout for None --, the two lengths as
    int64 device tensors or None)."""
    import torch

    S = _planes("x", x)
    B, C, T = x.shape
    if not same_frames and (not isinstance(other, torch.Tensor) or other.dim() != 3):
        raise ValueError(f"{name} must be a float32 device tensor [B, C or 1, K]")
    K = T if same_frames else other.shape[2]
    So = _planes(name, other, B, K, (C, 1) if C != 1 else (1,))
    if other.device != x.device:
        raise ValueError(f"x and {name} must be on one device")
    if x.numel() and K == 0:
        raise ValueError(f"{name} must have at least one frame")
    if out is not None and out is not x and (
            not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
            or (x.numel() and (_lines(out) is None or _lines(out)[0] != S))):
        raise ValueError("out must be x itself or a float32 tensor of x's shape, layout and device")
    for who, lens, most in (("lengths", lengths, T), (f"{name}_lengths", other_lengths, K)):
        if lens is not None and not isinstance(lens, torch.Tensor):
            _lengths_host(who, lens, B, most)
        elif lens is not None and (lens.dtype.is_floating_point or lens.dtype == torch.bool or lens.shape != (B,)):
            raise ValueError(f"{who} must be {B} integers")
    if x.numel() and out is not None:
        (x0, x1), (c0, c1), (o0, o1) = _span(x, S), _span(other, So), _span(out, S)
        if x0 != o0 and x0 < o1 and o0 < x1:
            raise ValueError("out overlaps x without being x")
        if c0 < o1 and o0 < c1:
            raise ValueError(f"{name} overlaps out")
    if out is None:
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    return (S, So, out, _lengths_device("lengths", lengths, B, x.device),
            _lengths_device(f"{name}_lengths", other_lengths, B, x.device))
