"""SpecAugment on log-mel features, behind the normalisations: a time warp, frequency masks and time masks per crop in one
launch (alacgpu_specaugment_device, csrc/alac_augment.hip).  Park et al. 2019; the time masks are bounded by a share of the
crop's length as in its adaptive form (Park et al. 2020).

The data is x float32 [B, C, M, N], M mel bins and N frames; a line is x[b, c, m, :].  With tau = min(max(lengths[b], 0), N)
(N without lengths) the stage touches the frames below tau only: everything at and behind tau, and every row with a length
<= 0, stays bit for bit.  All channels of a crop share its draws, three int32 tensors: warp [B, 2] = (c, c'), freq [B, F, 2]
and time [B, T, 2] = (first, width).  Within a crop, in this order:

  warp   only where 1 <= c, c' <= tau - 2 and c != c' ((0, 0) is no warp; c == c' is the identity).  Source frame c goes to
         frame c' and the two ends stay: frame t reads the source position
             s(t) = t c / c'                                       for t <= c'
             s(t) = c + (t - c') (tau - 1 - c) / (tau - 1 - c')    for t >  c'
         so s(0) = 0, s(c') = c, s(tau - 1) = tau - 1.  i = floor(s) and the remainder r over the denominator den (c' or
         tau - 1 - c') are integers, computed exactly (64-bit products), and
             y[t] = x[i]                                           where r == 0: x[i + 1] is not read
             y[t] = x[i] + f (x[i + 1] - x[i]),  f = r / den       elsewhere; i + 1 <= tau - 1 there
  freq   mask k sets the bins first .. first + width - 1, cut to 0 .. M - 1, to `fill` over the frames below tau
  time   mask k sets the frames first .. first + width - 1, cut to 0 .. tau - 1, of every bin to `fill`

A width <= 0 is no mask; masks may overlap one another and override the warp.

`specaugment_host` is this in float64 on the float32 input.  The kernel and `specaugment_host_f32` evaluate the warp in
float32: f = fl(fl(r) / fl(den)) -- r and den are integers below 2^24 wherever the kernel warps, so the two conversions are
exact and f is the correctly rounded quotient --, d = fl(x[i + 1] - x[i]), p = fl(f d), y = fl(x[i] + p): four roundings,
nothing contracted.  The twin is therefore the kernel bit for bit, whatever the layout.

The bound.  With u = 2^-24, m = max(|x[i]|, |x[i + 1]|) and no overflow or underflow, f' = f (1 + e1), d' = d (1 + e2),
p' = f' d' (1 + e3), |e_k| <= u, so |p' - f d| <= |f d| ((1 + u)^3 - 1) <= 2 m (3 u + 3 u^2 + u^3) as |f| < 1 and |d| <= 2 m.
The exact y = (1 - f) x[i] + f x[i + 1] is a convex combination, |y| <= m, so |x[i] + p'| <= m + 6.01 u m and the last rounding
adds at most u (1 + 6.01 u) m.  Together |y' - y| <= (7 u + 13 u^2) m < 8 u m:

    |twin - float64| <= 8 * 2^-24 * max(|x[i]|, |x[i + 1]|)        per warped element with r != 0; 0 elsewhere

for finite inputs whose differences do not overflow (|x| below 2^127) and whose products f d stay normal; the float64
statement's own rounding is 2^-29 of that.  Masked elements, untouched elements and warped elements with r == 0 are exact.
`specaugment_host(..., bound=True)` returns the bound next to the result.

Input that is not finite follows IEEE arithmetic: a NaN or an infinity in x[i] or x[i + 1] of a warped element with r != 0
reaches that element; with r == 0 only x[i] counts; one under a mask, or at or behind tau, is never read.

The draws (`SpecAugment.draw`) are made with torch on the device of the lengths, nothing read back, as `random_crops` and
`AddNoise.draw` draw: each is rand float64 [B] u mapped to lo + min(floor(u (span + 1)), span).  Their number and order are
fixed by the two mask counts alone, whatever the other parameters: 3 + 2 freq_masks + 2 time_masks calls,
    keep (u < p); warp c in W + 1 .. tau - 2 - W; warp shift in -W .. W, c' = c + shift (only where W > 0 and tau > 2 W + 2);
    per frequency mask its width in 0 .. min(freq_width, M), then its first bin in 0 .. M - width;
    per time mask its width in 0 .. min(time_width, floor(time_ratio tau)), then its first frame in 0 .. tau - width.
A crop that is not kept, or whose length is <= 0, gets zeros throughout.

`SpecAugment`, `specaugment_host` and `specaugment_host_f32` need no device.  `spec_augment` is the call on device tensors;
`Corpus.crops(augment=)` and `Corpus.random_crops(augment=)` run it last, behind `normalize=`.
"""
import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_device, _lengths_host, _lines, _Spec

_U = 2.0 ** -24
# csrc/alac_augment.h
WAVE_MAX, LDS_MAX, MAX_MASKS = 256, 16384, 1024


def _count(name, v, most=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0 or (most is not None and v > most):
        raise ValueError(f"{name} must be an integer in 0 .. {'' if most is None else most}, not {v!r}")
    return int(v)


class SpecAugment(_Spec):
    """SpecAugment's policy: freq_masks frequency masks of up to freq_width bins, time_masks time masks of up to
    min(time_width, floor(time_ratio * valid frames)) frames, a time warp of up to time_warp frames (0: none); masked
    elements become `fill` (0 is the line's mean behind a MeanVar); p is the probability that a crop is augmented at all.
    Immutable.  ValueError: a count or a width that is not a non-negative integer (the counts at most 1024, the widths and
    the warp below 2^31), time_ratio or p outside 0 .. 1, a fill that is not finite in float32."""

    __slots__ = ("freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "time_warp", "fill", "p")

    def __init__(self, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0, time_warp=0, fill=0.0, p=1.0):
        s = object.__setattr__
        s(self, "freq_masks", _count("freq_masks", freq_masks, MAX_MASKS))
        s(self, "freq_width", _count("freq_width", freq_width, (1 << 31) - 1))
        s(self, "time_masks", _count("time_masks", time_masks, MAX_MASKS))
        s(self, "time_width", _count("time_width", time_width, (1 << 31) - 1))
        s(self, "time_warp", _count("time_warp", time_warp, (1 << 31) - 1))
        for name, v in (("time_ratio", time_ratio), ("p", p)):
            v = _f32_finite(name, v)
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must be in 0 .. 1, not {v!r}")
            s(self, name, v)
        s(self, "fill", _f32_finite("fill", fill))

    def draw(self, n_mels, feat_lengths, generator=None):
        """The draws for crops of n_mels bins and feat_lengths [B] frames (an integer tensor; as `crops(features=)` returns
        them; no upper clamp is applied, so give lengths that are at most the frames there are): (warp int32 [B, 2], freq
        int32 [B, freq_masks, 2], time int32 [B, time_masks, 2]) on feat_lengths' device, by torch operations only; nothing
        is read back.  The module docstring states the draws and their order.  generator: a torch.Generator of that device
        or of the CPU (the draws are then made there and uploaded); default: the device's own."""
        import torch

        M = _count("n_mels", n_mels, (1 << 31) - 1)
        if not isinstance(feat_lengths, torch.Tensor) or feat_lengths.dim() != 1 or feat_lengths.dtype.is_floating_point or \
                feat_lengths.dtype == torch.bool:
            raise ValueError("feat_lengths must be an integer tensor [B]")
        here = feat_lengths.device
        dev = generator.device if generator is not None else here
        B = feat_lengths.shape[0]
        i64 = torch.int64
        tau = feat_lengths.to(i64).clamp(min=0)

        def uniform(span):
            """min(floor(u (span + 1)), span) for a fresh u, span int64 [B] >= 0"""
            u = torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here)
            return torch.minimum(torch.floor(u * (span + 1).to(torch.float64)).to(i64), span)

        zero = torch.zeros(B, dtype=i64, device=here)
        keep = (torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here) < self.p) & (tau > 0)
        W = self.time_warp
        c = W + 1 + uniform((tau - 3 - 2 * W).clamp(min=0))
        c1 = c - W + uniform(zero + 2 * W)
        warped = keep & (tau > 2 * W + 2) if W > 0 else keep & False
        warp = torch.where(warped[:, None], torch.stack([c, c1], dim=1), 0)
        pairs = []
        for count, most, room in ((self.freq_masks, zero + min(self.freq_width, M), zero + M),
                                  (self.time_masks, torch.floor(self.time_ratio * tau.to(torch.float64)).to(i64).clamp(max=self.time_width),
                                   tau)):
            made = []
            for _ in range(count):
                w = uniform(most)
                made.append(torch.stack([uniform(room - w), w], dim=1))
            t = torch.stack(made, dim=1) if made else torch.zeros((B, 0, 2), dtype=i64, device=here)
            pairs.append(torch.where(keep[:, None, None], t, 0).to(torch.int32))
        return warp.to(torch.int32), pairs[0], pairs[1]


# ---- the specification and its float32 twin ------------------------------------------------------------------------------------
def _host_args(x, warp, freq, time, lengths, fill):
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    if x.ndim != 4:
        raise ValueError(f"x must be [B, C, M, N], not {x.shape}")
    B, N = x.shape[0], x.shape[3]
    out = []
    for name, t, shape in (("warp", warp, (B, 2)), ("freq", freq, (B, None, 2)), ("time", time, (B, None, 2))):
        t = np.zeros((B, 2) if len(shape) == 2 else (B, 0, 2), dtype=np.int64) if t is None else np.asarray(t)
        if t.ndim != len(shape) or any(s is not None and s != k for s, k in zip(shape, t.shape)) or (t.size and t.dtype.kind not in "iu"):
            raise ValueError(f"{name} must be integers {list(shape)}, not {t.shape} {t.dtype}")
        out.append(t.astype(np.int64))
    return (x, *out, _lengths_host("lengths", lengths, B, N), np.float32(_f32_finite("fill", fill)))


def _source(tau, c, c1):
    """(i, r, den) int64 [tau] of a warp (c, c') of tau frames: the source position of frame t is i + r / den"""
    t = np.arange(tau, dtype=np.int64)
    left = t <= c1
    num = np.where(left, t * c, (t - c1) * (tau - 1 - c))
    den = np.where(left, c1, tau - 1 - c1)
    q = num // den
    return np.where(left, 0, c) + q, num - q * den, den


def _augment_host(x, warp, freq, time, lengths, fill, f32, bound):
    x, warp, freq, time, v, fill = _host_args(x, warp, freq, time, lengths, fill)
    B, C, M, N = x.shape
    y = x.copy() if f32 else x.astype(np.float64)
    dY = np.zeros(x.shape, dtype=np.float64) if bound else None
    with np.errstate(all="ignore"):
        for b in range(B):
            tau = int(v[b])
            if tau == 0:
                continue
            c, c1 = int(warp[b, 0]), int(warp[b, 1])
            if c != c1 and 1 <= c <= tau - 2 and 1 <= c1 <= tau - 2:
                i, r, den = _source(tau, c, c1)
                a, nxt = x[b, :, :, i], x[b, :, :, np.minimum(i + 1, tau - 1)]
                a, nxt = np.moveaxis(a, 0, -1), np.moveaxis(nxt, 0, -1)       # (an index array in front: numpy puts its axis first)
                if f32:
                    f = (r.astype(np.float32) / den.astype(np.float32)).astype(np.float32)
                    w = (a + (f * (nxt - a).astype(np.float32)).astype(np.float32)).astype(np.float32)
                else:
                    a, nxt = a.astype(np.float64), nxt.astype(np.float64)
                    w = a + (r / den) * (nxt - a)
                y[b, :, :, :tau] = np.where(r == 0, a, w)
                if bound:
                    dY[b, :, :, :tau] = np.where(r == 0, 0.0, 8 * _U * np.maximum(np.abs(a), np.abs(nxt)))
            for first, width in freq[b]:
                if width > 0:
                    lo, hi = max(int(first), 0), min(int(first + width), M)
                    if lo < hi:
                        y[b, :, lo:hi, :tau] = fill
                        if bound:
                            dY[b, :, lo:hi, :tau] = 0.0
            for first, width in time[b]:
                if width > 0:
                    lo, hi = max(int(first), 0), min(int(first + width), tau)
                    if lo < hi:
                        y[b, :, :, lo:hi] = fill
                        if bound:
                            dY[b, :, :, lo:hi] = 0.0
    return (y, dY) if bound else y


def specaugment_host(x, warp=None, freq=None, time=None, lengths=None, fill=0.0, bound=False):
    """The specification in numpy: x float32 [B, C, M, N] with the draws warp [B, 2], freq [B, F, 2], time [B, T, 2]
    (integers; None: none of that kind) to float64 of x's shape -- float64 arithmetic on the float32 input.  lengths: [B]
    integers (default N).  bound=True: returns (y, dY), dY float64 like y: how far the float32 evaluation may be from y (the
    module docstring)."""
    return _augment_host(x, warp, freq, time, lengths, fill, False, bound)


def specaugment_host_f32(x, warp=None, freq=None, time=None, lengths=None, fill=0.0):
    """The kernel's arithmetic in numpy, one float32 operation at a time: the same arguments to float32 of x's shape.  The
    kernel is held to it bit for bit."""
    return _augment_host(x, warp, freq, time, lengths, fill, True, False)


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _how(how, what="how"):
    """`how` as (SpecAugment or None, draws or None): a SpecAugment, the triple its `draw` returned, or the pair of both"""
    if isinstance(how, SpecAugment):
        return how, None
    if isinstance(how, tuple) and len(how) == 2 and isinstance(how[0], SpecAugment) and isinstance(how[1], tuple) and len(how[1]) == 3:
        return how
    if isinstance(how, tuple) and len(how) == 3 and what == "how":
        return None, how
    raise ValueError(f"{what} must be a SpecAugment{', the three tensors its draw() returned,' if what == 'how' else ''} or the pair "
                     f"(SpecAugment, draws), not {how!r}")


def _check_draws(draws, B, device):
    """The triple (warp or None, freq, time) as contiguous int32 tensors [B, 2], [B, F, 2], [B, T, 2] on `device`"""
    import torch

    out = []
    for name, t, dims in (("warp", draws[0], 2), ("freq", draws[1], 3), ("time", draws[2], 3)):
        if t is None and name == "warp":
            out.append(None)
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != dims or t.shape[0] != B or t.shape[-1] != 2:
            raise ValueError(f"the {name} draws must be an int32 tensor [{B}, {'' if dims == 2 else 'masks, '}2]")
        if t.device != device:
            raise ValueError(f"the {name} draws must be on {device}, not {t.device}")
        if dims == 3 and t.shape[1] > MAX_MASKS:
            raise ValueError(f"{t.shape[1]} {name} masks: at most {MAX_MASKS}")
        out.append(t.contiguous())
    return out


def _spec_augment(ctx, x, how, lengths, out, generator=None):
    """`spec_augment` behind its first check; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`),
    asked for behind the checks"""
    import torch

    spec, draws = _how(how)
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("x must be a float32 device tensor [B, C, M, N]")
    layout = _lines(x) if x.numel() else (max(x.shape[-1], 1), x.shape[-1])
    if layout is None:
        raise ValueError("x must be contiguous or the slice [..., :N] of a contiguous tensor")
    S, N = layout
    B, C, M = x.shape[:3]
    if out is not None and out is not x and (
            not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
            or (x.numel() and _lines(out) != layout)):
        raise ValueError("out must be x itself or a float32 tensor of x's shape, layout and device")
    d_valid = _lengths_device("lengths", lengths, B, x.device)
    if draws is not None:
        warp, freq, time = _check_draws(draws, B, x.device)
    if spec is not None and spec.time_warp == 0:
        warp = None                                 # (no warp can have been drawn: nothing is staged, no line is too long)
    elif draws is None or warp is not None:
        if N > LDS_MAX:
            raise ValueError(f"lines of {N} frames: a time warp takes at most {LDS_MAX}")
    if draws is None:
        tau = torch.full((B,), N, dtype=torch.int64, device=x.device) if d_valid is None else d_valid.clamp(max=N)
        drawn = spec.draw(M, tau, generator=generator)
        warp, freq, time = (None if spec.time_warp == 0 else drawn[0]), drawn[1], drawn[2]
    if out is None:
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    if x.numel() == 0:
        return out
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ctx().specaugment_device(x, out, B, C, M, S, N, d_valid, warp, freq if freq.shape[1] else None, time if time.shape[1] else None,
                                 0.0 if spec is None else spec.fill, stream=stream)
    return out


def spec_augment(x, how, lengths=None, out=None):
    """SpecAugment on the GPU: x float32 [B, C, M, N] on the device, contiguous or the slice [..., :N] of a contiguous tensor
    (what lies behind the slice is neither read nor written).  how: a `SpecAugment`, whose draws are then made here from the
    device's default generator; the pair (SpecAugment, draws) with the three tensors its `draw(M, lengths)` returned; or
    those three alone (warp or None, freq, time), which mask with a fill of 0.  lengths: [B] integers, a sequence or a tensor
    (the feat_lengths `crops` returns; -1 counts as 0, more than N as N): the frames of a crop that are signal, which alone are
    warped and masked; default: N.  out: x itself (in place; a crop that is not warped is then written where it is masked and
    nowhere else) or a tensor of x's shape and layout; default: a new one of x's layout.  Returns out.  One launch,
    asynchronous on the current stream; ValueError before any device work: anything else, draws of another shape, dtype or
    device, a time warp of lines longer than 16384 frames."""
    ctx = _device_context("x", x, "[B, C, M, N]")
    return _spec_augment(ctx, x, how, lengths, out)
