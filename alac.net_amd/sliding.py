"""Sliding-window cepstral mean (and variance) normalisation behind the features: Kaldi's `apply-cmvn-sliding` in one launch
(alacgpu_normalize_sliding_device, csrc/alac_sliding.hip), the third kind of `normalize`'s `how`.  Neither Kaldi nor
torchaudio is at hand where this is built: the parity is with this written specification, Kaldi's
`SlidingWindowCmnInternal` restated, not with foreign fixtures.

The data is float32 [B, ..., n]; a line is the last dimension, v = min(max(lengths[b], 0), n) its valid frames (n without
lengths).  SlidingMeanVar(window, min_window, center, norm_vars): frame t < v is normalised over the window [s, e), Kaldi's
with its quirks -- the non-centred window behind frame `window` is window + 1 frames long:

    center:      s = t - window // 2;  e = s + window
    otherwise:   s = t - window;       e = t + 1
    if s < 0:                 e -= s;  s = 0
    if not center and e > t:  e = max(t + 1, min_window)
    if e > v:                 s -= e - v;  e = v;  s = max(s, 0)
    N = e - s

    m    = (sum of x[s .. e)) / N
    y[t] = x[t] - m                                             without norm_vars
    y[t] = 0                            where N == 1,           with norm_vars
    y[t] = (x[t] - m) / sqrt(max(var, 1e-10)),  var = (sum of x[s .. e)^2) / N - m^2      otherwise
    y[t] = 0                            for v <= t < n

v = 0 -- a length of -1, a crop outside the corpus, included -- is a line of zeros and reads nothing.  `sliding_host` is this
in float64 with every window summed on its own (the variance as the mean of (x - m)^2, which is the same number); 1e-10 is
the float32 nearest to it.

The float32 arithmetic of the kernel, which `sliding_host_f32` follows one IEEE operation at a time, nothing contracted,
divisions and roots correctly rounded:

  pivot     p = fl(P / fl(v)), P the sum over [0, v) in `MeanVar`'s order (normalize._tree_p: 64 partial sums for n <= 256,
            1024 above) of the elements that are finite -- one that is not counts as +0, so that it reaches its windows and
            nothing else.  d[t] = fl(x[t] - p), and everything below works on d: a mean and a variance do not change under a
            shift, and E[d^2] - m^2 does not cancel on features with a large offset, such as c0.
  blocks    frames in blocks of 32 aligned at multiples of 32 from the line's start; a block's sum is a tree of halves
            (q[j] += q[j + h], h = 16 .. 1) over its 32 elements, those at or behind v counting as +0; the same over
            fl(d * d) with norm_vars.
  windows   with j0 = ceil(s / 32), j1 = floor(e / 32), one chain of additions from zero: the head elements s .. 32 j0 - 1
            ascending, the blocks j0 .. j1 - 1 ascending, the tail elements 32 j1 .. e - 1 ascending; where j0 >= j1 all
            elements ascending.  S1 over d, S2 over fl(d * d).
  result    m = fl(S1 / fl(N)), y = fl(d - m); with norm_vars var = max(fl(fl(S2 / fl(N)) - fl(m * m)), 1e-10f) and
            y = fl(fl(d - m) / sqrt(var)).

A window sum is a sum of that window's elements and of blocks inside it, never a difference of running sums: its error
depends on N, not on t or n.  With u = 2^-24, gamma_k = k u / (1 - k u), D_i = x_i - p exactly, M = mean D over the window,
Y = D_t - M (= x_t - m), any order of the window sums stays within

    dm   = gamma_{N+2} mean|D_i|                                   d's rounding, N - 1 additions, the division
    dd_t = (1 + u) (u |D_t| + dm) + u |Y|                          the computed d_t - m: both operands, one rounding
    dV   = (1 + u) (gamma_{N+3} mean(D_i^2) + 2 |M| dm + dm^2 + u (|M| + dm)^2) + u var
                                                                   the squares and their sum, the square of m, the difference
    ds   = dV / (2 s_lo) + 2 u s,   s = sqrt(max(var, 1e-10)),  s_lo = sqrt(max(var - dV, 1e-10))     (the floor is 1-Lipschitz)
    dY_t = dd_t / s_lo + |Y| ds / (s s_lo) + 4 u |y_t|             the numerator, the denominator, the division

of the exact value, as in normalize.py's chain; without norm_vars dY_t = dd_t, and where N == 1 with norm_vars y and dY are 0.
The bound is in terms of the pivot: un-pivoted, |D| is |x| and the bound of E[x^2] - m^2 on 30 + 1e-2 noise is larger than
the variance itself.  `sliding_host(..., bound=True)` returns dY for the pivot above.

What is not finite follows IEEE arithmetic: a NaN or an infinity at t0 < v reaches exactly the frames whose window holds t0
(their block and window sums), one at or behind v is never read.  A constant window has var = 0 or a rounding's worth of it,
floored at 1e-10: the result is finite.

`SlidingMeanVar`, `sliding_windows`, `sliding_host` and `sliding_host_f32` need no device; normalize.normalize is the call
on device tensors.
"""
import numpy as np

from ._stageargs import _lengths_host, _Spec, _tree

_U = 2.0 ** -24
BLOCK = 32                        # ALAC_SLIDING_BLOCK of csrc/alac_sliding.h
WAVE_MAX = 256                    # ALAC_SLIDING_WAVE_MAX: up to here the pivot has 64 partial sums, above 1024 (normalize.WAVE_MAX)
LDS_MAX = 16384                   # ALAC_SLIDING_LDS_MAX: up to here a line is held whole, above a ring of that many frames
RING_WINDOW_MAX = 7648            # ALAC_SLIDING_RING_WINDOW_MAX: the widest window of a line above LDS_MAX
VAR_FLOOR = np.float32(1e-10)


def _count(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1 or int(v) >= 1 << 31:
        raise ValueError(f"{name} must be an integer of 1 .. 2^31 - 1, not {v!r}")
    return int(v)


class SlidingMeanVar(_Spec):
    """Kaldi's sliding-window CMVN (SlidingWindowCmnOptions, its defaults): every frame minus the mean of a window of `window`
    frames around it (center) or behind it, of at least `min_window` frames at the start of a line when not centred; with
    norm_vars divided by the window's standard deviation.  Immutable.  ValueError: window or min_window not an integer >= 1,
    min_window > window, a flag that is not a boolean."""

    __slots__ = ("window", "min_window", "center", "norm_vars")

    def __init__(self, window=600, min_window=100, center=False, norm_vars=False):
        s = object.__setattr__
        window, min_window = _count("window", window), _count("min_window", min_window)
        if min_window > window:
            raise ValueError(f"min_window {min_window} is above window {window}")
        if not isinstance(center, (bool, np.bool_)) or not isinstance(norm_vars, (bool, np.bool_)):
            raise ValueError("center and norm_vars must be booleans")
        s(self, "window", window)
        s(self, "min_window", min_window)
        s(self, "center", bool(center))
        s(self, "norm_vars", bool(norm_vars))

    @classmethod
    def xvector(cls):
        """apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300: the Kaldi x-vector recipes'"""
        return cls(window=300, center=True)


def sliding_windows(v, how):
    """(s, e), int64 [v]: the window [s[t], e[t]) of every frame t of a line of v valid frames (the module docstring's lines)"""
    t = np.arange(v, dtype=np.int64)
    if how.center:
        s = t - how.window // 2
        e = s + how.window
    else:
        s = t - how.window
        e = t + 1
    neg = s < 0
    e = np.where(neg, e - s, e)
    s = np.where(neg, 0, s)
    if not how.center:
        e = np.where(e > t, np.maximum(t + 1, how.min_window), e)
    over = e > v
    s = np.maximum(np.where(over, s - (e - v), s), 0)
    e = np.where(over, v, e)
    return s, e


def _host_args(x, how, lengths):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 2:
        raise ValueError(f"x must be float32 [B, ..., n], not {x.dtype} {x.shape}")
    if not isinstance(how, SlidingMeanVar):
        raise ValueError(f"how must be a SlidingMeanVar, not {how!r}")
    return x, _lengths_host("lengths", lengths, x.shape[0], x.shape[-1])


def _pivot(X, n):
    """The kernel's pivot of the lines X [lines, v] float32 of a tensor whose lines have n elements: [lines, 1] float32"""
    from .normalize import _LANES, _LINE_THREADS, _tree_p

    f32 = np.float32
    t = np.where(np.isfinite(X), X, f32(0.0))
    return (_tree_p(t, _LANES if n <= WAVE_MAX else _LINE_THREADS) / f32(X.shape[1])).astype(f32)


def sliding_host(x, how, lengths=None, bound=False):
    """The specification in numpy: x float32 [B, ..., n] to float64 of that shape -- float64 arithmetic on the float32 input,
    every window summed on its own.  lengths: [B] integers (below 0 counts as 0, above n as n); default: whole lines.
    bound=True: returns (y, dY), dY float64 like y: how far a float32 evaluation that pivots as the kernel does may be from y
    (the module docstring's chain)."""
    from numpy.lib.stride_tricks import sliding_window_view

    x, lens = _host_args(x, how, lengths)
    shape = x.shape
    n = shape[-1]
    y = np.zeros(shape, dtype=np.float64)
    dY = np.zeros(shape, dtype=np.float64) if bound else None
    floor = float(VAR_FLOOR)
    with np.errstate(all="ignore"):
        for b in range(shape[0]):
            v = int(lens[b])
            if v == 0:
                continue
            X32 = x[b].reshape(-1, n)[:, :v]
            X = X32.astype(np.float64)
            lines = X.shape[0]
            D = X - _pivot(X32, n).astype(np.float64) if bound else None
            s, e = sliding_windows(v, how)
            N = e - s
            out = np.zeros((lines, v))
            err = np.zeros((lines, v)) if bound else None
            for Nu in np.unique(N):
                Nu = int(Nu)
                frames = np.nonzero(N == Nu)[0]
                view = sliding_window_view(X, Nu, axis=1)                       # [lines, v - Nu + 1, Nu]
                dview = sliding_window_view(D, Nu, axis=1) if bound else None
                step = max(1, (1 << 22) // (lines * Nu))
                for k in range(0, len(frames), step):
                    at = frames[k:k + step]
                    W = view[:, s[at], :]
                    m = W.mean(axis=-1)
                    Y = X[:, at] - m
                    var = ((W - m[..., None]) ** 2).mean(axis=-1)
                    sd = np.sqrt(np.maximum(var, floor))
                    if how.norm_vars:
                        res = np.zeros_like(Y) if Nu == 1 else Y / sd
                    else:
                        res = Y
                    out[:, at] = res
                    if not bound:
                        continue
                    Wd = dview[:, s[at], :]
                    g2, g3 = (Nu + 2) * _U / (1 - (Nu + 2) * _U), (Nu + 3) * _U / (1 - (Nu + 3) * _U)
                    M = Wd.mean(axis=-1)
                    dm = g2 * np.abs(Wd).mean(axis=-1)
                    dd = (1 + _U) * (_U * np.abs(D[:, at]) + dm) + _U * np.abs(Y)
                    if not how.norm_vars:
                        err[:, at] = dd
                    elif Nu > 1:
                        dV = (1 + _U) * (g3 * (Wd * Wd).mean(axis=-1) + 2 * np.abs(M) * dm + dm * dm + _U * (np.abs(M) + dm) ** 2) + _U * var
                        s_lo = np.sqrt(np.maximum(var - dV, floor))
                        ds = dV / (2 * s_lo) + 2 * _U * sd
                        err[:, at] = dd / s_lo + np.abs(Y) * ds / (sd * s_lo) + 4 * _U * np.abs(res)
            y[b].reshape(-1, n)[:, :v] = out
            if bound:
                dY[b].reshape(-1, n)[:, :v] = err
    return (y, dY) if bound else y


def _chain(acc, src, first, count):
    """acc [lines, v] float32 plus src[:, first[t] + k] for k = 0 .. count[t] - 1 in ascending k, one float32 addition each"""
    for k in range(int(count.max()) if len(count) else 0):
        on = k < count
        at = np.where(on, first + k, 0)
        acc = np.where(on[None, :], (acc + src[:, at]).astype(np.float32), acc)
    return acc


def sliding_host_f32(x, how, lengths=None):
    """The kernel's arithmetic in numpy, bit for bit: x float32 [B, ..., n] to float32 of that shape, the pivot, the block sums
    and the window chains of the module docstring, one float32 operation at a time"""
    x, lens = _host_args(x, how, lengths)
    f32 = np.float32
    shape = x.shape
    n = shape[-1]
    y = np.zeros(shape, dtype=f32)
    with np.errstate(all="ignore"):
        for b in range(shape[0]):
            v = int(lens[b])
            if v == 0:
                continue
            X = x[b].reshape(-1, n)[:, :v]
            lines = X.shape[0]
            d = (X - _pivot(X, n)).astype(f32)
            blocks = -(-v // BLOCK)
            pad = np.zeros((lines, blocks * BLOCK), dtype=f32)
            pad[:, :v] = d
            s, e = sliding_windows(v, how)
            N = e - s
            j0, j1 = -(-s // BLOCK), e // BLOCK
            split = j0 < j1
            head = np.where(split, BLOCK * j0 - s, N)
            sums = []
            for src in (pad, (pad * pad).astype(f32))[:2 if how.norm_vars else 1]:
                acc = _chain(np.zeros((lines, v), dtype=f32), src, s, head)
                acc = _chain(acc, _tree(src.reshape(lines, blocks, BLOCK)), j0, np.where(split, j1 - j0, 0))
                sums.append(_chain(acc, src, BLOCK * j1, np.where(split, e - BLOCK * j1, 0)))
            fN = N.astype(f32)[None, :]
            m = (sums[0] / fN).astype(f32)
            out = (d - m).astype(f32)
            if how.norm_vars:
                var = np.maximum(((sums[1] / fN).astype(f32) - (m * m).astype(f32)).astype(f32), VAR_FLOOR)
                out = np.where(N[None, :] == 1, f32(0.0), (out / np.sqrt(var).astype(f32)).astype(f32))
            y[b].reshape(-1, n)[:, :v] = out
    return y
