"""Sample-rate conversion behind the decode: a polyphase Hann-windowed sinc (alacgpu_resample_device, csrc/alac_resample.hip).

Source rate r, target rate R, g = gcd(r, R), a = r / g, b = R / g.  Rolloff 0.99 and Z = 6 zero crossings: f = 0.99 * min(a, b),
width = ceil(Z * a / f).  A signal x[0 .. T), zero outside, resamples to Ty = ceil(b * T / a) frames

    y[j] = sum over s of h(s / a - j / b) * x[s]
    h(u) = (f / a) * sinc(f * u) * cos^2(pi * f * u / (2 Z))   for |f * u| < Z, else 0

With j = i + b * m (phase i, period m) the tap at s = m * a + d has the weight w[i][d] = h(d / a - i / b); it is non-zero only
for |d - i * a / b| < Z * a / f <= width, so the N = 2 * width + 1 taps from d0[i] = floor(i * a / b) - width on hold all of
them, and output j reads the source frames floor(j * a / b) - width .. + N.  (The filter torchaudio.functional.resample uses by
default, with only the non-zero taps kept.)

`resample_table`, `resample_host` (the kernel's specification in numpy), `source_window` and `rows_tables` (the tables of a
call whose rows have different source rates, alacgpu_resample_rows_device) need no device.  `resample` is the
call on device tensors.
"""
import math

import numpy as np

ROLLOFF = 0.99
ZERO_CROSSINGS = 6
MAX_TABLE = 16384       # weights of a table: 64 KiB of LDS


def _ratio(orig_rate, new_rate):
    for name, v in (("orig_rate", orig_rate), ("new_rate", new_rate)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) <= 0:
            raise ValueError(f"{name} must be a positive integer, not {v!r}")
    r, R = int(orig_rate), int(new_rate)
    g = math.gcd(r, R)
    return r // g, R // g


def filter_width(a, b):
    """width = ceil(Z * a / f), f = 0.99 * min(a, b): the filter's reach in source frames"""
    return int(math.ceil(ZERO_CROSSINGS * a / (ROLLOFF * min(a, b))))


def _table(a, b, width):
    """(d0[b] int32, weights[b, N] float32) of the ratio a : b: computed in float64, rounded once"""
    N = 2 * width + 1
    f = ROLLOFF * min(a, b)
    i = np.arange(b, dtype=np.int64)
    d0 = (i * a) // b - width
    d = d0[:, None] + np.arange(N, dtype=np.int64)[None, :]
    # u = d / a - i / b as one exact integer over a * b: s / a - j / b of the closed form is the same integer over a * b
    t = f * ((d * b - i[:, None] * a).astype(np.float64) / (a * b))
    w = (f / a) * np.sinc(t) * np.cos(np.pi * t / (2 * ZERO_CROSSINGS)) ** 2
    w[np.abs(t) >= ZERO_CROSSINGS] = 0.0
    return d0.astype(np.int32), w.astype(np.float32)


def resample_table(orig_rate, new_rate):
    """The polyphase table of orig_rate -> new_rate: (a, b, width, d0[b] int32, weights[b, N] float32), N = 2 * width + 1.
    Phase i's taps are the source frames m * a + d0[i] .. + N of period m; a row's taps outside the filter's support have
    weight zero.  ValueError: a rate that is not a positive integer, or a table of more than 16384 weights (it has to fit
    64 KiB of LDS)."""
    a, b = _ratio(orig_rate, new_rate)
    width = filter_width(a, b)
    N = 2 * width + 1
    if b * N > MAX_TABLE:
        raise ValueError(f"{orig_rate} Hz to {new_rate} Hz is a = {a}, b = {b}: a table of {b} x {N} = {b * N} weights, "
                         f"the kernel holds at most {MAX_TABLE}")
    d0, w = _table(a, b, width)
    return a, b, width, d0, w


def identity_table():
    """The table that copies: a = b = 1 with one tap of weight 1 between two of weight 0 (the kernel wants width >= 1).  What
    `mono` alone runs through the kernel; the filter of equal rates is never built."""
    return 1, 1, 1, np.array([-1], dtype=np.int32), np.array([[0.0, 1.0, 0.0]], dtype=np.float32)


def rows_tables(rates, new_rate):
    """The tables of a call with a table per row (alacgpu_resample_rows_device) for sources of the sample rates `rates` that
    all go to new_rate: one table per distinct reduced ratio, in the order the ratios first appear, a source already at
    new_rate with `identity_table`.  Returns (table_of int64 [len(rates)]: a source's table, desc uint32 [n_tables, 5]: a, b,
    width and where the table's d0 and weights start in the two arrays, d0 int32: the tables' d0 one behind the other,
    weights float32: their weights, flat).  ValueError: a rate that is not a positive integer; a table of more than 16384
    weights, naming the first source that needs it."""
    index, desc, d0s, ws, table_of = {}, [], [], [], []
    n_d0 = n_w = 0
    for f, rate in enumerate(rates):
        a, b = _ratio(rate, new_rate)
        if (a, b) not in index:
            try:
                a, b, width, d0, w = identity_table() if a == b else resample_table(rate, new_rate)
            except ValueError as e:
                raise ValueError(f"source {f}: {e}") from None
            index[(a, b)] = len(desc)
            desc.append((a, b, width, n_d0, n_w))
            d0s.append(d0.reshape(-1))
            ws.append(w.reshape(-1))
            n_d0, n_w = n_d0 + d0.size, n_w + w.size
        table_of.append(index[(a, b)])
    return (np.asarray(table_of, dtype=np.int64), np.asarray(desc, dtype=np.uint32).reshape(-1, 5),
            np.concatenate(d0s).astype(np.int32) if d0s else np.zeros(0, np.int32),
            np.concatenate(ws).astype(np.float32) if ws else np.zeros(0, np.float32))


def source_window(o, L, a, b, width):
    """The source frames the target frames o .. o + L need: (s0, Ls) with s0 = (o // b) * a - width, the first one (it may be
    negative), and Ls = ((L - 1) // b + 2) * a + 2 * width, the frames to reserve from s0 on -- a bound that depends on L and
    the rates only, so a batch of crops shares it."""
    o, L = int(o), int(L)
    return (o // b) * a - width, ((L - 1) // b + 2) * a + 2 * width


def resampled_frames(T, a, b):
    """Ty = ceil(b * T / a) (numpy arrays too)"""
    return (b * T + a - 1) // a


def apply_table(x, a, b, width, d0, weights, mono=False, origin=0, first=0, num_frames=None, magnitude=False):
    """alacgpu_resample_device on the host, in numpy: x float64 [..., C, T] (or [T]) holds the source frames origin ..
    origin + T of a signal that is zero everywhere else; returns the target frames first .. first + num_frames (default: up
    to the signal's end) as float64.  The float32 weights widened to float64, float64 accumulation in ascending d.  A target
    frame outside 0 .. ceil(b * (origin + T) / a) is zero: the resampled signal ends there.  mono: (x[0] + x[1]) * 0.5 in
    float32 first, the channel axis stays with length 1.  magnitude: sum |w * x| instead -- what the error bound of a float32
    evaluation is a multiple of."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    if mono and x.ndim >= 2 and x.shape[-2] == 2:
        x32 = x.astype(np.float32)
        x = ((x32[..., 0:1, :] + x32[..., 1:2, :]) * np.float32(0.5)).astype(np.float64)
    elif mono and (x.ndim < 2 or x.shape[-2] != 1):
        raise ValueError(f"mono takes [..., 1 or 2, T], not {x.shape}")
    end = resampled_frames(origin + T, a, b)
    if num_frames is None:
        num_frames = max(end - first, 0)
    N = 2 * width + 1
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(b, N)
    d0 = np.asarray(d0).astype(np.int64)
    if magnitude:
        x, w = np.abs(x), np.abs(w)
    y = np.zeros(x.shape[:-1] + (num_frames,), dtype=np.float64)
    taps = np.arange(N, dtype=np.int64)
    for lo in range(0, num_frames, 1 << 16):
        j = first + np.arange(lo, min(lo + (1 << 16), num_frames), dtype=np.int64)
        i, m = j % b, j // b
        s = (m * a + d0[i])[:, None] + taps[None, :] - origin          # [n, N]: where in x
        inside = (s >= 0) & (s < T)
        xs = np.where(inside, x[..., np.clip(s, 0, max(T - 1, 0))] if T else 0.0, 0.0)
        acc = np.zeros(x.shape[:-1] + (len(j),), dtype=np.float64)
        for k in range(N):
            acc = acc + w[i, k] * xs[..., k]
        acc[..., (j < 0) | (j >= end)] = 0.0
        y[..., lo:lo + len(j)] = acc
    return y


def resample_host(x, orig_rate, new_rate, mono=False, magnitude=False):
    """The kernel's specification for a whole signal: x float64 [..., T] at orig_rate, zero outside 0 .. T, to new_rate --
    ceil(b * T / a) frames, float64 (`apply_table` with the rates' table from frame 0 on).  mono: [..., C, T] to
    [..., 1, ceil(b * T / a)].  Equal rates return x (its mono sum with `mono`)."""
    a, b = _ratio(orig_rate, new_rate)
    table = identity_table() if a == b else resample_table(orig_rate, new_rate)
    return apply_table(x, *table, mono=mono, magnitude=magnitude)


# ---- on the device -------------------------------------------------------------------------------------------------------------
_TABLES = {}     # (a, b, device index) -> (a, b, width, d_d0, d_weights)
_CONTEXTS = {}   # device index -> the AlacGpuContext `resample` launches through (the call uses nothing of it but its device)


def device_table(orig_rate, new_rate, device):
    """The table of orig_rate -> new_rate on the device (a torch.device), uploaded once per ratio and device: (a, b, width,
    d_d0 int32, d_weights float32).  Equal rates give the identity table."""
    import torch

    a, b = _ratio(orig_rate, new_rate)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (a, b, index)
    if key not in _TABLES:
        a, b, width, d0, w = identity_table() if a == b else resample_table(orig_rate, new_rate)
        dev = torch.device("cuda", index)
        _TABLES[key] = (a, b, width, torch.from_numpy(d0).to(dev), torch.from_numpy(w).to(dev))
    return _TABLES[key]


def _context(index):
    from . import AlacGpuContext

    if index not in _CONTEXTS:
        _CONTEXTS[index] = AlacGpuContext([(4096, 16, 40, 10, 14, 2)], index)
    return _CONTEXTS[index]


def resample(pcm, orig_rate, new_rate, lengths=None, mono=False):
    """Resample PCM on the GPU: pcm float32 [C, T] or [F, C, T] on the device (as `load` and `load_batch` return it), C 1 or
    2, from orig_rate to new_rate with the filter of this module; asynchronous on the current stream.  [C, T] returns the
    tensor [C or 1, ceil(b * T / a)].  [F, C, T] returns (tensor [F, C or 1, ceil(b * T / a)], new lengths): `lengths`
    (load_batch's: a sequence or an int64 tensor, default T for every file) are the files' frames -- what lies behind them
    counts as zero, and so does what lies behind the new lengths ceil(b * lengths / a), an int64 tensor where `lengths` was.
    mono: the mean of two channels, taken in float32 in front of the filter.  Equal rates without `mono` return pcm itself
    (and lengths) and launch nothing."""
    import torch

    from . import _VP

    if not isinstance(pcm, torch.Tensor) or pcm.device.type != "cuda" or pcm.dtype != torch.float32 or pcm.dim() not in (2, 3):
        raise ValueError("pcm must be a float32 device tensor [C, T] or [F, C, T]")
    a, b = _ratio(orig_rate, new_rate)
    batch = pcm.dim() == 3
    if lengths is not None and not batch:
        raise ValueError("lengths belong to a batch [F, C, T]")
    F, C_, T = (pcm.shape if batch else (1,) + tuple(pcm.shape))
    if C_ not in (1, 2):
        raise ValueError(f"{C_} channels: the resampler takes 1 or 2")
    dev = pcm.device
    if lengths is None:
        lens = torch.full((F,), T, dtype=torch.int64)
    else:
        lens = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths, dtype=np.int64))
        if lens.shape != (F,) or lens.dtype.is_floating_point:
            raise ValueError(f"lengths must be {F} integers")
        lens = lens.to(torch.int64)
    if a == b and not (mono and C_ == 2):
        return (pcm, lens) if batch else pcm
    a, b, width, d_d0, d_w = device_table(orig_rate, new_rate, dev)
    Ty = resampled_frames(T, a, b)
    new_lens = resampled_frames(lens.clamp(0, T), a, b)
    out = torch.empty((F, 1 if mono else C_, Ty), dtype=torch.float32, device=dev)
    if F and Ty:
        zeros = torch.zeros(F, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _context(dev.index).resample_device(pcm.contiguous(), F, C_, T, zeros, lens.clamp(0, T).to(dev), zeros, Ty, a, b, width,
                                                d_d0, d_w, mono, out, stream=torch.cuda.current_stream(dev).cuda_stream)
    return (out, new_lens) if batch else out[0]
