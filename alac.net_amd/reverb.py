"""Room reverberation into crops, on the waveform and in front of the noise mix (alacgpu_reverb_device, csrc/alac_reverb.hip).

A row is a crop x[b] float32 [C, T] with its room impulse response h[b] float32 [Ch, K], Ch = C or 1 (one channel of the
response goes into every channel of the signal).  With v = min(max(lengths[b], 0), T), vh = min(max(rir_lengths[b], 0), K)
(T and K without them),

    d = the first k < vh at which |h[0, k]| is largest      the direct path; channel 0 decides, so a two-channel response keeps
                                                            its delay between the channels
    e = (sum over c < Ch, k < vh of h[c, k]^2) / Ch,   g = 1 / sqrt(e)        a response of unit energy; one gain for every
                                                            channel, so a two-channel response keeps its level difference
    y[c, i] = g * sum over k < vh of h[c mod Ch, k] * x[c, i + d - k]    for i < v, x taken as 0 outside 0 .. v
    y[c, i] = x[c, i]                                                    for v <= i < T (in place: untouched)

The result is as long as the crop and aligned on the direct path; the tail behind v is dropped; lengths stay.  A row is x bit
for bit, and only this decision reads its response, where v == 0, where vh == 0 -- how "no reverberation for this crop" is
expressed --, where e == 0 (a silent response) or where e is not finite; e is taken as the kernel has it, in float32.  What
is not finite is never hidden: a NaN or an infinity in x[b, :, :v] may reach any element below v of that row and no element
of another (one in h[b, :, :vh] makes e not finite: the row stays); one at or behind v (vh) is never read.

The kernel's scheme (csrc/alac_reverb.h), which `reverb_host_f32` follows operation for operation: a uniformly partitioned
overlap-save convolution with blocks of N = 4096 frames at a hop of H = N / 2.  Block j of a signal plane holds
x[(j - 1) H + t], t < N (0 outside 0 .. v), j = 0 .. ceil(v / H); partition p of a response plane h[p H + t], t < H (0 at and
behind vh), p < P = ceil(vh / H).  Each is transformed as N complex points by a radix-4 decimation-in-frequency transform whose
twiddles exp(-2 pi i k / N) are computed in float64 and rounded once (`twiddles`); block m of w = h * x is elements H .. N of
the inverse transform of sum over p of X[m - p] . H[p], in ascending p, divided by N (exactly: a power of two), and
y[i] = g w[i + d].  A complex product is (ar br - ai bi, ar bi + ai br); every operation is one float32 operation, none fused.
e is summed as the header states: partial t of 256 takes the squares of the frames t, t + 256, ... below vh of channel 0, then
of channel 1; the 256 partials are added as a tree of halves; division and root are the correctly rounded ones.

The bound, derived, not measured.  u = 2^-24, gamma_k = k u / (1 - k u).  A radix-4 stage is two radix-2 stages of which one
has the exact twiddles 1 and -i, so the normwise bound of the radix-2 transform of log2 N = 12 stages covers it (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 24.2): the computed transform of z is F z + r with
||r||_2 <= f ||F z||_2 = f sqrt(N) ||z||_2,

    f = 12 eta / (1 - 12 eta),   eta = mu + gamma_4 (sqrt(2) + mu),   mu = u      (a twiddle's two parts are each rounded once
                                                                                   from float64: its error is at most u)

So with a_p = sqrt(N) ||x block m - p||_2 and b_p = sqrt(N) ||h partition p||_2 the computed spectra are within f a_p and
f b_p of the true ones in the 2-norm.  A float32 complex product has a relative error of at most cm = sqrt(2) gamma_2
(Higham, Lemma 3.5), and ||s . t||_2 <= ||s||_2 ||t||_2 for the element-wise product, so the computed product of partition p
is within a_p b_p phi of X . H, phi = (1 + f)^2 (1 + cm) - 1; the P - 1 float32 additions in ascending p add
gamma_P sum |products|, together psi = phi + gamma_P (1 + phi) times A = sum over p of a_p b_p.  The inverse transform of
the computed sum W' has the error f sqrt(N) ||W'||_2 <= f sqrt(N) (1 + psi) A of its own and carries the error of its input
with the norm sqrt(N) psi A; an element's error is at most the 2-norm of the block's.  The division by N is exact, and
A = N sum over p of ||x block m - p||_2 ||h partition p||_2, so for every n of block m

    |w'[n] - w[n]| <= Ew[m] = sqrt(N) kappa * sum over p of ||x block m - p||_2 ||h partition p||_2,
    kappa = psi + f (1 + psi)                               about 240 u + P u:  c(N, P) = sqrt(N) kappa / u is about 15600

and by Cauchy-Schwarz the sum is at most sqrt(P) ||h[c mod Ch]||_2 times the largest norm of a block of x that block m reads
(the frames (m - P) H .. (m + 1) H).  The gain: the float32 sum of M = Ch vh squares in any order is within gamma_M, the
division by Ch, the root and the reciprocal add u each and the root halves what is under it, so g' = g (1 + t),
|t| <= dg = gamma_{Ch vh} + 3 u.  The last product is rounded once:

    dY[c, i] = g (1 + dg)(1 + u) Ew[(i + d) div H] + (dg + u (1 + dg)) |y[c, i]|      for i < v of a row that is processed;
                                                                                       0 elsewhere (y is x exactly)

`reverb_host(..., bound=True)` returns dY.  It assumes that nothing underflows.  The bound is loose by design -- the norm of
a block stands for each of its elements --; the tests hold the kernel to a small multiple of what the float32 twin achieves.

`Reverb`, `reverb_host` and `reverb_host_f32` need no device.  `reverb` is the call on device tensors;
`Corpus.crops(reverb=)` and `Corpus.random_crops(reverb=)` put it between the waveform and `mix=`.
"""
import math

import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_host, _signal_and_companion, _Spec, _tree

_U = 2.0 ** -24
# csrc/alac_reverb.h
N, STAGES, THREADS = 4096, 6, 256
HOP = N // 2


def twiddles():
    """The kernel's table: (cos, -sin)(2 pi k / N), k < N, computed in float64 and rounded once to float32"""
    a = 2.0 * 3.14159265358979323846 * np.arange(N, dtype=np.float64) / float(N)
    return np.cos(a).astype(np.float32), (-np.sin(a)).astype(np.float32)


class Reverb(_Spec):
    """Room reverberation from a corpus of impulse responses or from simulated rooms, for `Corpus.crops(reverb=)` and
    `Corpus.random_crops(reverb=)`.  rirs: a `rir.ShoeboxRooms` -- every crop then gets the image-source response of a room
    drawn for it, one channel, max_seconds long (`rooms` is that policy, else None); a policy whose smallest room holds more
    than rir.LIMIT candidate images within max_seconds is refused here, and again at the crops' rate --, or an open `Corpus` on the device of the corpus whose crops it reverberates; its rate or rates and its channel count
    (1 or 2) may differ: the first max_seconds of the drawn file are taken at the rate of the crops, and as one channel when
    its channel count is not theirs.  p in 0 .. 1: the probability that a crop is reverberated at all.  max_seconds: a
    positive number.  Immutable.  ValueError otherwise."""

    __slots__ = ("rirs", "p", "max_seconds")

    def __init__(self, rirs, p=1.0, max_seconds=1.0):
        from .corpus import Corpus

        from .rir import ShoeboxRooms

        s = object.__setattr__
        if isinstance(rirs, ShoeboxRooms):
            pass
        elif not isinstance(rirs, Corpus):
            raise ValueError(f"rirs must be a Corpus or a ShoeboxRooms, not {rirs!r}")
        elif getattr(rirs, "_gpu", None) is None:
            raise ValueError("the corpus of impulse responses is closed")
        elif rirs.channels not in (1, 2):
            raise ValueError(f"a corpus of impulse responses has 1 or 2 channels, not {rirs.channels}")
        p = _f32_finite("p", p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be in 0 .. 1, not {p!r}")
        max_seconds = _f32_finite("max_seconds", max_seconds)
        if not max_seconds > 0.0:
            raise ValueError(f"max_seconds must be positive, not {max_seconds!r}")
        if isinstance(rirs, ShoeboxRooms):
            from .rir import LIMIT, box_candidates

            most = box_candidates(rirs.smallest(), max_seconds, rirs.sound_speed)
            if most > LIMIT and rirs.max_order is None:
                raise ValueError(f"the smallest room {rirs.smallest()!r} of {rirs!r} has {most:.3g} candidate images within "
                                 f"{max_seconds!r} s, more than {LIMIT}: every such row would be refused")
        s(self, "rirs", rirs)
        s(self, "p", p)
        s(self, "max_seconds", max_seconds)

    @property
    def rooms(self):
        """The ShoeboxRooms of a Reverb over simulated rooms, else None"""
        from .rir import ShoeboxRooms

        return self.rirs if isinstance(self.rirs, ShoeboxRooms) else None

    def check_rate(self, sample_rate):
        """ValueError where the smallest room of a Reverb over rooms is refused at `sample_rate`; nothing for a Corpus"""
        rooms = self.rooms
        if rooms is not None:
            from .rir import LIMIT, candidate_box

            low = rooms.smallest()
            geom = np.array(low + tuple(0.5 * v for v in low) * 2, dtype=np.float64)
            if candidate_box(geom, float(sample_rate) / rooms.sound_speed, self.frames(sample_rate), rooms.taps // 2,
                             -1 if rooms.max_order is None else rooms.max_order) is None:
                raise ValueError(f"the smallest room {low!r} of {rooms!r} has more than {LIMIT} candidate images in "
                                 f"{self.frames(sample_rate)} frames at {sample_rate} Hz: every such row would be refused")

    def frames(self, sample_rate):
        """K: the frames of a response at sample_rate, max(1, round(max_seconds * sample_rate))"""
        return max(1, int(round(self.max_seconds * sample_rate)))

    def draw(self, batch, generator=None, device=None):
        """The draws of `batch` crops as device tensors.  Over rooms: (geometry float64 [B, 9], beta float32 [B, 6], keep bool
        [B]) on `device` (which only this kind needs): the four draws of `ShoeboxRooms.draw` first, then rand float64 k, keep
        where k < p.  Over a corpus: (rir_files int64 [B], keep bool [B], False where the crop is not
        reverberated).  Two draws of B values, always in this order, whatever p is, so that a seeded generator reproduces
        them: the files (randint, uniform over the corpus of responses), then rand float64 k, keep where k < p.  generator:
        a torch.Generator of the corpus's device or of the CPU (the draws are then made there and uploaded); default: the
        device's own.  Nothing is read back."""
        import torch

        from . import _frame_count

        rirs = self.rirs
        if self.rooms is not None:
            B = _frame_count("batch", batch)
            if device is None:
                raise ValueError("the draws of a Reverb over rooms need device=")
            geometry, beta = rirs.draw(B, generator=generator, device=device)
            dev = generator.device if generator is not None else device
            keep = (torch.rand(B, generator=generator, device=dev, dtype=torch.float64) < self.p).to(device)
            return geometry, beta, keep
        if rirs._gpu is None:
            raise ValueError("the corpus of impulse responses is closed")
        if rirs.num_files == 0:
            raise ValueError("the corpus of impulse responses is empty")
        B = _frame_count("batch", batch)
        here = rirs._dev
        dev = generator.device if generator is not None else here
        files = torch.randint(0, rirs.num_files, (B,), generator=generator, device=dev, dtype=torch.int64).to(here)
        keep = (torch.rand(B, generator=generator, device=dev, dtype=torch.float64) < self.p).to(here)
        return files, keep


# ---- the specification and its float32 twin ------------------------------------------------------------------------------------
def _host_args(x, rir, lengths, rir_lengths):
    x, rir = np.asarray(x), np.asarray(rir)
    if x.dtype != np.float32 or rir.dtype != np.float32:
        raise ValueError(f"x and rir must be float32, not {x.dtype} and {rir.dtype}")
    if x.ndim != 3 or x.shape[1] == 0 or x.shape[2] == 0:
        raise ValueError(f"x must be [B, C, T], not {x.shape}")
    B, C, T = x.shape
    if rir.ndim != 3 or rir.shape[0] != B or rir.shape[2] == 0 or rir.shape[1] not in (1, C):
        raise ValueError(f"rir must be [{B}, {C} or 1, K], not {rir.shape}")
    return x, rir, _lengths_host("lengths", lengths, B, T), _lengths_host("rir_lengths", rir_lengths, B, rir.shape[2])


def _sum_squares(h):
    """The kernel's float32 sum of the squares of h float32 [Ch, vh], in csrc/alac_reverb.h's order"""
    Ch, vh = h.shape
    rounds = -(-vh // THREADS)
    t = np.zeros((Ch, rounds * THREADS), dtype=np.float32)            # (a frame at or behind vh adds +0: nothing)
    t[:, :vh] = (h * h).astype(np.float32)
    q = np.zeros(THREADS, dtype=np.float32)
    for c in range(Ch):
        for r in range(rounds):
            q = (q + t[c, r * THREADS:(r + 1) * THREADS]).astype(np.float32)
    return _tree(q)


def _verdict(h, k, kh):
    """(d, g as float32) of a row's response h float32 [Ch, K] with kh valid frames, or None where the row is left alone"""
    if k == 0 or kh == 0:
        return None
    with np.errstate(all="ignore"):
        e = np.float32(_sum_squares(h[:, :kh]) / np.float32(h.shape[0]))
        if not (e > 0 and e < np.inf):
            return None
        g = np.float32(np.float32(1) / np.float32(np.sqrt(e)))
    return int(np.argmax(np.abs(h[0, :kh]))), g


def _block_norms(a, count, first):
    """||a[first(j) .. first(j) + span]||_2 in float64 for j < count, (first, span) = `first`"""
    origin, span = first
    a = a.astype(np.float64)
    out = np.zeros(count)
    for j in range(count):
        lo, hi = max(origin(j), 0), min(origin(j) + span, a.shape[0])
        if lo < hi:
            out[j] = np.sqrt(np.sum(a[lo:hi] ** 2))
    return out


def kappa(parts):
    """kappa of the module docstring for `parts` partitions: c(N, P) = sqrt(N) * kappa / u"""
    gam = lambda k: k * _U / (1 - k * _U)
    eta = _U + gam(4) * (math.sqrt(2.0) + _U)
    stages = 2 * STAGES
    f = stages * eta / (1 - stages * eta)
    phi = (1 + f) ** 2 * (1 + math.sqrt(2.0) * gam(2)) - 1
    psi = phi + gam(parts) * (1 + phi)
    return psi + f * (1 + psi)


def reverb_host(x, rir, lengths=None, rir_lengths=None, bound=False):
    """The specification in numpy: x float32 [B, C, T] and rir float32 [B, Ch, K] (Ch = C or 1) to float64 [B, C, T] -- float64
    arithmetic on the float32 inputs, by direct summation.  lengths, rir_lengths: [B] integers (default T and K).
    bound=True: returns (y, dY), dY float64 like y: how far a float32 evaluation in the kernel's scheme may be from y (the
    module docstring)."""
    x, rir, v, vh = _host_args(x, rir, lengths, rir_lengths)
    B, C, T = x.shape
    Ch = rir.shape[1]
    y = x.astype(np.float64)
    dY = np.zeros(x.shape, dtype=np.float64)
    gam = lambda k: k * _U / (1 - k * _U)
    with np.errstate(all="ignore"):
        for b in range(B):
            k, kh = int(v[b]), int(vh[b])
            if _verdict(rir[b], k, kh) is None:
                continue
            h = rir[b, :, :kh].astype(np.float64)
            d = int(np.argmax(np.abs(h[0])))
            root = np.sqrt((h * h).sum() / Ch)                                # g w as w / sqrt(e): one tap a gives sign(a) x exactly
            g = 1.0 / root
            parts = -(-kh // HOP)
            for c in range(C):
                hc = h[c % Ch]
                w = np.convolve(x[b, c, :k].astype(np.float64), hc)           # direct summation; w[n], n < k + kh - 1
                y[b, c, :k] = w[d:d + k] / root
                if bound:
                    nx = _block_norms(x[b, c, :k], -(-k // HOP) + 1, (lambda j: (j - 1) * HOP, N))
                    nh = _block_norms(hc, parts, (lambda p: p * HOP, HOP))
                    Ew = math.sqrt(N) * kappa(parts) * np.convolve(nx, nh)      # [m]: sum over p of nx[m - p] nh[p]
                    dg = gam(Ch * kh) + 3 * _U
                    m = (np.arange(k) + d) // HOP
                    dY[b, c, :k] = g * (1 + dg) * (1 + _U) * Ew[m] + (dg + _U * (1 + dg)) * np.abs(y[b, c, :k])
    return (y, dY) if bound else y


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1]), (a[0] * b[1] + a[1] * b[0])


def _butterflies(L):
    q = np.arange(N // 4)
    j = q & (L - 1)
    i0 = ((q - j) << 2) + j
    step = N // (4 * L)
    return (i0, i0 + L, i0 + 2 * L, i0 + 3 * L), (j * step, 2 * j * step, 3 * j * step)


def _forward(zr, zi, tw):
    """The kernel's forward transform of [n, N] float32 (real and imaginary parts) in place: base-4 digit-reversed order out"""
    L = N // 4
    while L >= 1:
        (i0, i1, i2, i3), ks = _butterflies(L)
        a, b, c, d = ((zr[:, i], zi[:, i]) for i in (i0, i1, i2, i3))
        t0, t1, t2 = (a[0] + c[0], a[1] + c[1]), (a[0] - c[0], a[1] - c[1]), (b[0] + d[0], b[1] + d[1])
        bd = (b[0] - d[0], b[1] - d[1])
        t3 = (bd[1], -bd[0])
        outs = ((t0[0] + t2[0], t0[1] + t2[1]), (t1[0] + t3[0], t1[1] + t3[1]), (t0[0] - t2[0], t0[1] - t2[1]), (t1[0] - t3[0], t1[1] - t3[1]))
        zr[:, i0], zi[:, i0] = outs[0]
        for i, o, k in zip((i1, i2, i3), outs[1:], ks):
            zr[:, i], zi[:, i] = _cmul(o, (tw[0][k], tw[1][k]))
        L //= 4


def _inverse(zr, zi, tw):
    """The kernel's inverse transform, not divided by N: digit-reversed order in, natural order out"""
    L = 1
    while L <= N // 4:
        (i0, i1, i2, i3), ks = _butterflies(L)
        z0 = (zr[:, i0], zi[:, i0])
        z1, z2, z3 = (_cmul((zr[:, i], zi[:, i]), (tw[0][k], -tw[1][k])) for i, k in zip((i1, i2, i3), ks))
        u0, u1, u2 = (z0[0] + z2[0], z0[1] + z2[1]), (z0[0] - z2[0], z0[1] - z2[1]), (z1[0] + z3[0], z1[1] + z3[1])
        dz = (z1[0] - z3[0], z1[1] - z3[1])
        u3 = (-dz[1], dz[0])
        outs = ((u0[0] + u2[0], u0[1] + u2[1]), (u1[0] + u3[0], u1[1] + u3[1]), (u0[0] - u2[0], u0[1] - u2[1]), (u1[0] - u3[0], u1[1] - u3[1]))
        for i, o in zip((i0, i1, i2, i3), outs):
            zr[:, i], zi[:, i] = o
        L *= 4


def _spectra(blocks, tw):
    zr = np.ascontiguousarray(blocks, dtype=np.float32)
    zi = np.zeros_like(zr)
    _forward(zr, zi, tw)
    return zr, zi


def reverb_host_f32(x, rir, lengths=None, rir_lengths=None):
    """The kernel's scheme in numpy float32, one operation at a time: the same blocks, partitions, transform, twiddle values,
    order of the partitions and of the sum of squares (csrc/alac_reverb.h): x float32 [B, C, T], rir float32 [B, Ch, K] to
    float32 [B, C, T].  Its distance from `reverb_host` is what a correct float32 evaluation of this scheme costs: the tests
    hold the kernel to a small multiple of that."""
    x, rir, v, vh = _host_args(x, rir, lengths, rir_lengths)
    f32 = np.float32
    B, C, T = x.shape
    Ch = rir.shape[1]
    y = x.copy()
    tw = twiddles()
    with np.errstate(all="ignore"):
        for b in range(B):
            k, kh = int(v[b]), int(vh[b])
            verdict = _verdict(rir[b], k, kh)
            if verdict is None:
                continue
            d, g = verdict
            last_x, parts = -(-k // HOP), -(-kh // HOP)
            hb = np.zeros((Ch, parts, N), dtype=f32)
            for c in range(Ch):
                for p in range(parts):
                    seg = rir[b, c, p * HOP:min((p + 1) * HOP, kh)]
                    hb[c, p, :seg.shape[0]] = seg
            Hr, Hi = (s.reshape(Ch, parts, N) for s in _spectra(hb.reshape(-1, N), tw))
            padded = np.zeros((C, (last_x + 2) * HOP), dtype=f32)              # x[(j - 1) H + t] at j H + t
            padded[:, HOP:HOP + k] = x[b, :, :k]
            xb = np.stack([padded[:, j * HOP:j * HOP + N] for j in range(last_x + 1)], axis=1)
            Xr, Xi = (s.reshape(C, last_x + 1, N) for s in _spectra(xb.reshape(-1, N), tw))
            ms = np.arange(d // HOP, (d + k - 1) // HOP + 1)
            for c in range(C):
                ar, ai = np.zeros((len(ms), N), dtype=f32), np.zeros((len(ms), N), dtype=f32)
                for n, m in enumerate(ms):
                    for p in range(max(m - last_x, 0), min(m, parts - 1) + 1):
                        pr, pi = _cmul((Xr[c, m - p], Xi[c, m - p]), (Hr[c % Ch, p], Hi[c % Ch, p]))
                        ar[n], ai[n] = ar[n] + pr, ai[n] + pi
                _inverse(ar, ai, tw)
                w = (ar[:, HOP:] * f32(1.0 / N)).reshape(-1)                   # w[n], n from ms[0] H
                first = d - int(ms[0]) * HOP
                y[b, c, :k] = g * w[first:first + k]
    return y


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _reverb(ctx, x, rir, lengths, rir_lengths, out):
    """`reverb` behind its first checks; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`), asked
    for behind the checks"""
    import torch

    S, Sh, out, d_valid, d_rir_valid = _signal_and_companion(x, "rir", rir, lengths, rir_lengths, out, same_frames=False)
    if x.numel() == 0:
        return out
    B, C, T = x.shape
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ctx().reverb_device(x, out, rir, B, C, rir.shape[1], S, Sh, T, rir.shape[2], d_valid, d_rir_valid, stream=stream)
    return out


def reverb(x, rir, lengths=None, rir_lengths=None, out=None):
    """Room reverberation into a batch on the GPU: x float32 [B, C, T] and rir float32 [B, Ch, K] (Ch = C or 1) on one
    device, each contiguous or the slice [..., :T] ([..., :K]) of a contiguous tensor (what lies behind the slice is neither
    read nor written).  Every row is convolved with its response, aligned on the response's largest tap and scaled by the
    response's energy (the module docstring).  lengths, rir_lengths: [B] integers, sequences or tensors (as `crops` returns
    them; -1 counts as 0, more than T or K as T or K): the frames of a row that are signal and of its response that are
    response; a response of 0 frames leaves the row as it is, bit for bit; default: T and K.  out: x itself (in place) or a
    tensor of x's shape and layout that neither x nor rir overlaps; default: a new one of x's layout.  Returns out.  Two
    launches, asynchronous on the current stream; ValueError before any device work."""
    return _reverb(_device_context("x", x, "[B, C, T]"), x, rir, lengths, rir_lengths, out)
