"""Noise at a target signal-to-noise ratio into crops, on the waveform and in front of the features (alacgpu_mix_device,
csrc/alac_mix.hip).

A row is a crop x[b] float32 [C, T] with its noise n[b] float32 [Cn, T], Cn = C or 1 (one noise channel goes into every
channel of the signal).  With v = min(max(lengths[b], 0), T), vn = min(max(noise_lengths[b], 0), T) (T without them) and
a = ratio[b], the float32 amplitude ratio 10^(-snr_db / 20):

    Ps   = (sum over c, i < v  of x[c, i]^2) / fl(C * v)
    Pn   = (sum over c, i < vn of n[c, i]^2) / fl(Cn * vn)      over the noise's own valid frames, not the repeated ones
    g    = fl(a * fl(sqrt(fl(Ps / Pn))))                         but g = 0 where a == 0, v == 0, vn == 0 or Pn == 0
    y[c, i] = fl(x[c, i] + fl(g * n[c mod Cn, i mod vn]))   for i < v      noise shorter than the crop is repeated
    y[c, i] = x[c, i]                                       for v <= i < T (in place: untouched)

and where g == 0, by those four conditions or by the formula (Ps == 0), the row's noise is not read and y is x bit for bit.
That is how a crop that draws "no noise" is expressed (ratio 0; `mix` maps a NaN in snr_db to it), and why a silent noise clip
(Pn == 0) cannot turn a batch into NaN.  The decibels are not the kernel's: a power of ten is not correctly rounded, so the
stage would stop being specifiable; `mix` computes the ratio with torch on the device.

The kernel evaluates this in float32, one IEEE operation at a time, none fused, the divisions and the root correctly rounded
and the counts C * v and Cn * vn converted with one rounding.  The sums are float32 in a fixed order (csrc/alac_mix.h), which
`mix_host_f32` follows: a row is cut into parts of PART = 4096 frames (the smallest multiple of 4096 that keeps a row within
MAX_PARTS = 256 parts), the same parts for the signal and the noise.  Within the part that begins at frame f0, partial j of
ROUND = 1024 is ((0 + t[0, f0 + j]) + t[0, f0 + j + ROUND]) + ... over the part's frames below v (vn), channel 0 first, then
channel 1 likewise, t the squares rounded once.  The 4 partials of a thread (j = 4 thread + k) are added as a tree of halves
(q[k] += q[k + h], h = 2, 1), the 64 sums of a wave by the same tree (h = 32 .. 1), the 4 wave sums by the same tree
(h = 2, 1), and the parts of a row in ascending order, ((0 + S[0]) + S[1]) + ...  The order does not depend on the width of
the kernel's loads, so the twin is the kernel bit for bit on every layout.

The bound.  All terms of both sums are non-negative, so with u = 2^-24, gamma_k = k u / (1 - k u), N = C v and M = Cn vn a
float32 sum of squares in ANY order is S (1 + t), |t| <= gamma_N (one rounding of a square and at most N - 1 additions on the
way of any term), and Ps', Pn' carry two roundings more (the count and the division): relative errors within g1 = gamma_{N+2}
and g2 = gamma_{M+2}.  The quotient r' = fl(Ps' / Pn') is then between r (1 - g1)(1 - u) / (1 + g2) >= r (1 - e) and
r (1 + g1)(1 + u) / (1 - g2) = r (1 + e'), e = g1 + g2 + u, e' = (g1 + g2 + u + g1 u) / (1 - g2).  A root halves a relative
error upwards, sqrt(1 + e') <= 1 + e' / 2, and does not double it downwards, sqrt(1 - e) >= 1 - e; the root and the product
with a add (1 +- u)^2.  Downwards that is 1 - e - 2 u = 1 - (g1 + g2 + 3 u); upwards, while g1, g2 <= 1/4 (N, M below
3.3 million), e' / 2 <= (2/3)(g1 + g2) + 0.84 u and (1 + e' / 2)(1 + u)^2 <= 1 + (2/3)(g1 + g2) + 3.6 u.  So the relative error
of g is at most

    dg   = gamma_{C v + 2} + gamma_{Cn vn + 2} + 4 u                          whatever the order of the sums

with at least 0.4 u to spare.  The product g' n_i has one rounding, |fl(g' n_i) - g n_i| <= E_i = |g n_i| (dg + u (1 + dg)),
and the sum with x_i one more, u (|y_i| + E_i); the u E_i of it is below the 0.4 u |g n_i| dg has to spare:

    dY_i = |g n_i| (dg + u (1 + dg)) + u |y_i|          for i < v of a row with g != 0;  0 elsewhere (y is x exactly)

`mix_host(..., bound=True)` returns dY.  It assumes that no square underflows (|x|, |n| above 2^-63 or 0).

Input that is not finite follows IEEE arithmetic and is never hidden: a NaN or an infinity inside x[.., :v], or inside
n[.., :vn] of a row with a != 0, v != 0 and vn != 0, reaches that row and no other; one at or behind v (vn) is never read.  A
negative, infinite or NaN ratio is data like any other.

`AddNoise`, `mix_host` and `mix_host_f32` need no device.  `mix` is the call on device tensors; `Corpus.crops(mix=)` and
`Corpus.random_crops(mix=)` put it between the waveform and `features=`.
"""

import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_host, _signal_and_companion, _Spec, _tree

_U = 2.0 ** -24
# csrc/alac_mix.h
PART, MAX_PARTS, ROUND, VEC = 4096, 256, 1024, 4
_LANES, _THREADS = 64, 256


def part_frames(frames):
    """alac_mix_part_frames: the frames of a part of a row of `frames` frames"""
    least = -(-frames // PART)
    return PART * max(-(-least // MAX_PARTS), 1)


class AddNoise(_Spec):
    """Noise from a second corpus at a signal-to-noise ratio drawn per crop, for `Corpus.crops(mix=)` and
    `Corpus.random_crops(mix=)`.  noise: an open `Corpus` on the device of the corpus it is mixed into -- that corpus itself
    will do; its rate and channel count may differ (the noise is cropped at the rate of the crops, and as one channel when its
    channel count is not theirs).  snr_db: a finite number, or (lo, hi) with lo <= hi: uniform in lo .. hi per crop.  p in
    0 .. 1: the probability that a crop gets noise at all.  Immutable; snr_db is kept as (lo, hi).  ValueError otherwise."""

    __slots__ = ("noise", "snr_db", "p")

    def __init__(self, noise, snr_db, p=1.0):
        from .corpus import Corpus

        s = object.__setattr__
        if not isinstance(noise, Corpus):
            raise ValueError(f"noise must be a Corpus, not {noise!r}")
        if getattr(noise, "_gpu", None) is None:
            raise ValueError("the noise corpus is closed")
        if isinstance(snr_db, (tuple, list)):
            if len(snr_db) != 2:
                raise ValueError(f"snr_db must be a number or (lo, hi), not {snr_db!r}")
            lo, hi = _f32_finite("snr_db[0]", snr_db[0]), _f32_finite("snr_db[1]", snr_db[1])
            if lo > hi:
                raise ValueError(f"snr_db {snr_db!r}: lo above hi")
        else:
            lo = hi = _f32_finite("snr_db", snr_db)
        p = _f32_finite("p", p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be in 0 .. 1, not {p!r}")
        s(self, "noise", noise)
        s(self, "snr_db", (lo, hi))
        s(self, "p", p)

    def draw(self, batch, num_frames, sample_rate=None, generator=None):
        """The draws of `batch` crops of num_frames frames at sample_rate (default: the noise corpus's own rate), as device
        tensors: (noise_files int64 [B], noise_offsets int64 [B], snr_db float32 [B], NaN where the crop gets no noise).
        Drawn as `Corpus.random_crops` draws, four draws of B values each in this order, whatever snr_db and p are, so that a
        seeded generator reproduces them: the files (randint, uniform over the noise corpus), the offsets (rand float64 u,
        floor(u (span + 1)) with span = max(T_f - num_frames, 0) at sample_rate), the ratio (rand float64 s, lo + (hi - lo) s
        rounded to float32), and whether there is noise (rand float64 k, noise where k < p).  generator: a torch.Generator of
        the corpus's device or of the CPU (the draws are then made there and uploaded); default: the device's own.
        Nothing is read back."""
        import torch

        from . import _frame_count

        noise = self.noise
        if noise._gpu is None:
            raise ValueError("the noise corpus is closed")
        if noise.sample_rate is None and sample_rate is None:
            raise ValueError("the files of the noise corpus differ in sample rate: the draws need sample_rate=")
        if noise.num_files == 0:
            raise ValueError("the noise corpus is empty")
        B, L = _frame_count("batch", batch), _frame_count("num_frames", num_frames)
        here = noise._dev
        dev = generator.device if generator is not None else here
        rand = lambda: torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here)
        files = torch.randint(0, noise.num_files, (B,), generator=generator, device=dev, dtype=torch.int64).to(here)
        u = rand()
        totals = noise._d_num_frames if sample_rate is None else noise._rate(sample_rate)["d_Ty"]
        span = (totals[files] - L).clamp(min=0)
        offs = torch.minimum(torch.floor(u * (span + 1).to(torch.float64)).to(torch.int64), span)
        lo, hi = self.snr_db
        snr = (lo + (hi - lo) * rand()).to(torch.float32)
        snr = torch.where(rand() < self.p, snr, float("nan"))
        return files, offs, snr


# ---- the specification and its float32 twin ------------------------------------------------------------------------------------
def _host_args(x, noise, ratio, lengths, noise_lengths):
    x, noise = np.asarray(x), np.asarray(noise)
    if x.dtype != np.float32 or noise.dtype != np.float32:
        raise ValueError(f"x and noise must be float32, not {x.dtype} and {noise.dtype}")
    if x.ndim != 3 or x.shape[1] == 0:
        raise ValueError(f"x must be [B, C, T], not {x.shape}")
    B, C, T = x.shape
    if noise.ndim != 3 or noise.shape[0] != B or noise.shape[2] != T or noise.shape[1] not in (1, C):
        raise ValueError(f"noise must be [{B}, {C} or 1, {T}], not {noise.shape}")
    a = np.asarray(ratio)
    if a.shape != (B,) or (B and a.dtype.kind not in "fiu"):
        raise ValueError(f"ratio must be {B} numbers, not {a.shape} {a.dtype}")
    with np.errstate(all="ignore"):
        a = a.astype(np.float32)
    return x, noise, a, _lengths_host("lengths", lengths, B, T), _lengths_host("noise_lengths", noise_lengths, B, T)


def _tiled(n, C, v, vn):
    """n [Cn, T] as the noise of every frame below v of C channels: n[c mod Cn, i mod vn]"""
    return n[np.arange(C) % n.shape[0]][:, np.arange(v) % vn]


def mix_host(x, noise, ratio, lengths=None, noise_lengths=None, bound=False):
    """The specification in numpy: x float32 [B, C, T], noise float32 [B, Cn, T] (Cn = C or 1) and ratio [B] (as float32) to
    float64 [B, C, T] -- float64 arithmetic on the float32 inputs.  lengths, noise_lengths: [B] integers (default T).
    bound=True: returns (y, dY), dY float64 like y: how far a float32 evaluation may be from y (the module docstring)."""
    x, noise, a, v, vn = _host_args(x, noise, ratio, lengths, noise_lengths)
    B, C, T = x.shape
    Cn = noise.shape[1]
    y = x.astype(np.float64)
    dY = np.zeros(x.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            k, kn, ab = int(v[b]), int(vn[b]), float(a[b])
            if ab == 0.0 or k == 0 or kn == 0:
                continue
            X, N = x[b, :, :k].astype(np.float64), noise[b, :, :kn].astype(np.float64)
            Ps, Pn = (X * X).sum() / (C * k), (N * N).sum() / (Cn * kn)
            if Pn == 0.0:
                continue
            g = ab * np.sqrt(Ps / Pn)
            if g == 0.0:
                continue
            gn = g * _tiled(N, C, k, kn)
            y[b, :, :k] = X + gn
            if bound:
                g1, g2 = ((m + 2) * _U / (1 - (m + 2) * _U) for m in (C * k, Cn * kn))
                dg = g1 + g2 + 4 * _U
                dY[b, :, :k] = np.abs(gn) * (dg + _U * (1 + dg)) + _U * np.abs(y[b, :, :k])
    return (y, dY) if bound else y


def _sum_squares(X, k):
    """The kernel's float32 sum of the squares of X[:, :k] (X float32 [channels, T]), in csrc/alac_mix.h's order"""
    f32 = np.float32
    channels, T = X.shape
    pf = part_frames(T)
    total = f32(0)
    for f0 in range(0, T, pf):
        end = min(f0 + pf, k)
        part = f32(0)
        if f0 < end:
            rounds = -(-(end - f0) // ROUND)
            t = np.zeros((channels, rounds * ROUND), dtype=f32)       # (a frame behind `end` adds +0: nothing)
            t[:, :end - f0] = (X[:, f0:end] * X[:, f0:end]).astype(f32)
            t = t.reshape(channels, rounds, ROUND)
            q = np.zeros(ROUND, dtype=f32)
            for c in range(channels):
                for r in range(rounds):
                    q = (q + t[c, r]).astype(f32)
            part = _tree(_tree(_tree(q.reshape(_THREADS, VEC)).reshape(_THREADS // _LANES, _LANES)))
        total = f32(total + part)
    return total


def mix_host_f32(x, noise, ratio, lengths=None, noise_lengths=None):
    """The kernel's arithmetic in numpy, one float32 operation at a time and the sums in the kernel's documented order: x
    float32 [B, C, T], noise float32 [B, Cn, T], ratio [B] to float32 [B, C, T].  Its distance from `mix_host` is what a
    correct float32 evaluation costs: the tests hold the kernel to a small multiple of that, and to the twin bit for bit."""
    x, noise, a, v, vn = _host_args(x, noise, ratio, lengths, noise_lengths)
    f32 = np.float32
    B, C, T = x.shape
    Cn = noise.shape[1]
    y = x.copy()
    with np.errstate(all="ignore"):
        for b in range(B):
            k, kn, ab = int(v[b]), int(vn[b]), a[b]
            if ab == 0 or k == 0 or kn == 0:
                continue
            Ps = f32(_sum_squares(x[b], k) / f32(C * k))
            Pn = f32(_sum_squares(noise[b], kn) / f32(Cn * kn))
            if Pn == 0:
                continue
            g = f32(ab * f32(np.sqrt(f32(Ps / Pn))))
            if g == 0:
                continue
            y[b, :, :k] = (x[b, :, :k] + (g * _tiled(noise[b], C, k, kn)).astype(f32)).astype(f32)
    return y


# ---- on the device -------------------------------------------------------------------------------------------------------------
def snr_ratio(snr_db, batch, device):
    """The amplitude ratio 10^(-snr_db / 20) as a float32 device tensor [batch]; 0 where snr_db is NaN.  snr_db: a number, a
    sequence or a tensor of `batch` numbers.  ValueError otherwise."""
    import torch

    if isinstance(snr_db, torch.Tensor):
        if snr_db.shape != (batch,) or snr_db.dtype in (torch.bool,) or snr_db.is_complex():
            raise ValueError(f"snr_db must be {batch} numbers")
        s = snr_db.to(device, torch.float32)
    else:
        try:
            arr = np.asarray(snr_db, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"snr_db must be a number or {batch} numbers, not {snr_db!r}") from None
        if isinstance(snr_db, (bool, np.bool_)) or arr.shape not in ((), (batch,)):
            raise ValueError(f"snr_db must be a number or {batch} numbers, not {snr_db!r}")
        s = torch.from_numpy(np.broadcast_to(arr, (batch,)).astype(np.float32)).to(device)
    return torch.where(s.isnan(), 0.0, torch.pow(10.0, s * (-1.0 / 20.0)))


def _mix(ctx, x, noise, ratio, lengths, noise_lengths, out):
    """`mix` behind its first checks; ratio() gives the ratio (a float32 device tensor [B]) and ctx() the context that runs it
    (the corpus's own inside `Corpus.crops`), both asked for behind the checks"""
    import torch

    S, Sn, out, d_valid, d_noise_valid = _signal_and_companion(x, "noise", noise, lengths, noise_lengths, out, same_frames=True)
    ratio = ratio()
    if x.numel() == 0:
        return out
    B, C, T = x.shape
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ctx().mix_device(x, out, noise, B, C, noise.shape[1], S, Sn, T, d_valid, d_noise_valid, ratio.contiguous(), stream=stream)
    return out


def mix(x, noise, snr_db, lengths=None, noise_lengths=None, out=None):
    """Noise into a batch on the GPU: x float32 [B, C, T] and noise float32 [B, Cn, T] (Cn = C or 1) on one device, each
    contiguous or the slice [..., :T] of a contiguous tensor (what lies behind the slice is neither read nor written).
    snr_db: the signal-to-noise ratio in decibels of every row, a number, a sequence or a tensor [B]; NaN: no noise for this
    row, which stays as it is bit for bit.  lengths, noise_lengths: [B] integers, sequences or tensors (as `crops` returns
    them; -1 counts as 0, more than T as T): the frames of a row that are signal -- they alone count for the power, get noise
    and, in the noise, are used, repeated where they are fewer; default: T.  out: x itself (in place) or a tensor of x's shape
    and layout that neither x nor noise overlaps; default: a new one of x's layout.  Returns out.  Two launches behind one
    small torch expression for the ratio, asynchronous on the current stream; ValueError before any device work."""
    ctx = _device_context("x", x, "[B, C, T]")
    return _mix(ctx, x, noise, lambda: snr_ratio(snr_db, x.shape[0], x.device), lengths, noise_lengths, out)
