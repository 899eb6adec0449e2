"""A crop brought to a known level, behind the noise and in front of the effects (alacgpu_level_device, csrc/alac_level.hip):
peak, RMS or ITU-R BS.1770-4 integrated loudness, so that a corpus put together from sources 25 dB apart reaches the model at
one level and a random gain perturbs around a target instead of an arbitrary centre.

A row is a crop x[b] float32 [C, T] with v = min(max(lengths[b], 0), T) (T without lengths); a `Level` says what to reach.
The kernel evaluates no logarithm and no power: every constant that needs one is computed here in float64 and handed over as
a linear number A (`Level.linear`), as mix.py hands over its amplitude ratio.  Everything below is float64 on x widened exactly.

    P = max |x[c, i]| over all channels and i < v                                  a NaN if there is one
    peak:  g = A / P                                            A = target
    rms:   E = (sum over c, i < v of x^2) / (C v),  g = sqrt(A / E)                A = 10^(db / 10)
    lufs:  every channel K-weighted by two biquad sections, `kweight(rate)`: highshelf(rate, 1500, 1/sqrt 2, +4 dB) and
           highpass(rate, 38, 0.5) of biquad.py's designers -- the RBJ forms pyloudnorm and torchaudio use at every rate; at
           48 kHz their magnitude response is within 0.044 dB of BS.1770's printed coefficient table over 20 Hz .. 20 kHz, 0.041 dB
           at 997 Hz, where a sine at 0 dBFS so reads -3.05 for the table's -3.01 (tests/test_level_spec.py measures it) -- each section from zero history, nothing rounded to float32, nothing clamped
           hop = floor(rate / 10 + 1/2) frames, a block is 4 hop frames, blocks start every hop: nh = v // hop whole hops and
           n_blocks = nh - 3 = (v - 4 hop) // hop + 1 (0 for v < 4 hop).  For rates that are multiples of 10 that is torchaudio's
           blocking (0.4 s, 75 % overlap); for the others a block is at most 2 frames off 0.4 s (hop is at most half a frame
           off a tenth of a second)
           s_c[k] = the sum of the squares of the weighted channel over hop k
           z_c[j] = ((s_c[j] + s_c[j+1]) + (s_c[j+2] + s_c[j+3])) / (4 hop)
           e[j]   = sum over c of G_c z_c[j],  G = (1, 1, 1, 1.41, 1.41)           more than 5 channels: ValueError
           m1     = the mean of the e[j] > Gabs,  Gabs = 10^((-70 + 0.691) / 10)   the absolute gate
           E      = the mean of the e[j] that are > Gabs and > 0.1 m1              the relative gate
           g      = sqrt(A / E)                                                    A = 10^((target + 0.691) / 10)
    max_peak:  g = m where m = max_peak / P is below g
    y[c, i] = fl32(g * x[c, i]) for i < v, rounded once; with `clamp` then min(max(y, -1), 1), a NaN staying a NaN

Frames at or behind v are untouched.  A row with nothing to measure keeps g = 1 exactly and is neither read by the second
launch nor written: v == 0, P == 0, E == 0, no block above the absolute gate, v < 4 hop for lufs.  A row whose g comes out
exactly 1 without clamp is treated the same way.  A NaN or an infinity below v is data and reaches its own row only: a NaN
peak or energy makes g a NaN, a block whose energy is a NaN is above no gate; one at or behind v is never read.
`level_host` is this in numpy with the sequential recurrence of `biquad_host` and numpy's own sums.

The kernel's order (csrc/alac_level.h), which `level_host_twin` follows operation by operation, nothing fused.  The measure
launch gives a (row, channel) to a workgroup of THREADS = 256 lanes, which walks it in tiles of TILE = 4096 frames, lane l the
CHUNK = 16 frames from 16 l on; a frame at or behind v counts as 0.
    the sum of squares: a lane's 16 squares (exact in float64) in ascending order from 0, the 64 lanes of a wave as a tree of
        halves (q[l] += q[l + h], h = 32 .. 1), the 4 waves likewise (h = 2, 1), the tiles in ascending order; the channels
        in ascending order from the first
    the K-weighting: the blocked recurrence of biquad.py (`biquad_host_twin`'s, 2 sections, gain 1), not rounded
    a hop sum: a chunk touches at most two hops (hop >= 16); its squares, rounded once, go in ascending order from 0 into one
        partial per hop it touches, and s[k] is the sum of the partials of hop k in ascending order of their chunks, from 0,
        whatever tile a chunk lies in.  A chunk that straddles a hop boundary -- 4410 and 1103 are no multiples of 16 -- so
        gives its first frames to the end of one sum and its last frames to the beginning of the next.  Frames at or behind
        nh hop are in no hop
    the blocks in ascending order; e[j] = G_0 z_0, then + G_c z_c in ascending order; both gated sums in ascending order from 0
    one correctly rounded division and root each, as written above
No sum is an atomic one and none depends on the width of the loads, so the same inputs give the same bits on every layout.

The bound on the twin's g against the specification's.  P is the same number in both.  Every term of S and of a hop sum is a
non-negative square, so with u = 2^-53 a float64 sum of N of them in ANY order is within N u of the exact one, relatively:
S and E of rms differ by at most 2 (C v + 2) u, 1.4e-11 for a million frames, and the root halves it.  For lufs the K-weighted
samples themselves differ: blocked against sequential by biquad.py's D, which for these two sections (poles at radius 0.99
at 8 kHz, 0.998 at 48 kHz: R below 3) is below 1e-12 of the channel's peak, but the gates are comparisons: a block whose
energy lies within that distance of a gate may pass in one evaluation and not in the other, and E then moves by up to a
block's share, orders above any rounding.  A derivation therefore says something only away from the gates, where it gives
|g_twin / g_host - 1| <= 1e-11; at a gate it says nothing, and the stage is held to what its number formats promise, as
biquad.py does: y is float32 and rounded once, so |g_twin / g_host - 1| <= 2^-24, one float32 rounding of the output.
Measured on the rows of tests/test_level_spec.py (8000 and 11025 Hz, two channels, lengths up to 8209): 0 for peak, 2.2e-16
for rms, at most 6.3e-15 and 1.9e-14 for lufs at the two rates.  The kernel is then within 2^-24 |s| + 2^-24 max |s| of
`level_host`'s s; measured on one MI355X on those rows: at most 4.5e-8 of the row's peak.

`Level`, `level_host`, `level_host_twin`, `loudness_host` and `kweight` need no device.  `level` and `loudness` are the calls
on device tensors; `Corpus.crops(level=)` and `Corpus.random_crops(level=)` run the stage behind mix= and in front of effects=.
"""
import functools
import math

import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_device, _lengths_host, _lines, _planes, _Spec
from .biquad import CHUNK, THREADS, TILE, _sequential, _twin_rows, highpass, highshelf

# csrc/alac_level.h
PEAK, RMS, LUFS = 0, 1, 2
MODES = ("peak", "rms", "lufs")
MAX_CHANNELS, MIN_HOP, HEAD, PART, MAX_PARTS, BATCH = 5, 16, 2, 4096, 256, 256
WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)
GATE_ABS = 1.1724653045822981e-07          # the double nearest 10^((-70 + 0.691) / 10): a literal, as the header's is
GATE_REL = 0.1
_LANES = 64
_OFFSET = 0.691                            # BS.1770's -0.691 dB
KWEIGHT_TABLE_DB = 0.044                    # kweight(48000) against BS.1770's printed table over 20 Hz .. 20 kHz, measured (dB)


# ---- the policy ----------------------------------------------------------------------------------------------------------------
class Level(_Spec):
    """What `level`, `Corpus.crops(level=)` and `Corpus.random_crops(level=)` bring a crop to: `Level.peak(target=1.0)` -- the
    largest magnitude of all channels becomes target --, `Level.rms(db=-25.0)` -- the mean square over all channels becomes
    db decibels re full scale -- or `Level.lufs(target=-23.0)` -- the BS.1770-4 integrated loudness becomes target LUFS.
    max_peak: the gain is lowered where the peak would otherwise pass it (a positive number; None: not limited).  clamp: the
    result is limited to -1 .. 1.  Immutable; `target` is the number given, `linear` what the kernel gets.  ValueError: a mode
    that is none of MODES, a target that is not finite (or not positive for peak, or whose power leaves float64), a max_peak
    that is not positive and finite, a clamp that is no bool."""

    __slots__ = ("mode", "target", "max_peak", "clamp")

    def __init__(self, mode, target, max_peak=None, clamp=False):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {', '.join(MODES)}, not {mode!r}")
        target = _f32_finite("target", target)
        if max_peak is not None:
            max_peak = _f32_finite("max_peak", max_peak)
            if not max_peak > 0.0:
                raise ValueError(f"max_peak must be positive, not {max_peak!r}")
        if not isinstance(clamp, (bool, np.bool_)):
            raise ValueError(f"clamp must be a bool, not {clamp!r}")
        s = object.__setattr__
        s(self, "mode", mode)
        s(self, "target", target)
        s(self, "max_peak", max_peak)
        s(self, "clamp", bool(clamp))
        if not (0.0 < self.linear < math.inf):
            raise ValueError(f"a {mode} target of {target!r} is not a positive finite number as a linear one")

    @classmethod
    def peak(cls, target=1.0, max_peak=None, clamp=False):
        return cls("peak", target, max_peak, clamp)

    @classmethod
    def rms(cls, db=-25.0, max_peak=None, clamp=False):
        return cls("rms", db, max_peak, clamp)

    @classmethod
    def lufs(cls, target=-23.0, max_peak=None, clamp=False):
        return cls("lufs", target, max_peak, clamp)

    @property
    def code(self):
        """The mode as the header counts it"""
        return MODES.index(self.mode)

    @property
    def linear(self):
        """A of the module docstring, float64, computed here: the peak, the mean square 10^(db / 10), or 10^((LUFS + 0.691) / 10)"""
        if self.mode == "peak":
            return self.target
        try:
            return math.pow(10.0, (self.target + (_OFFSET if self.mode == "lufs" else 0.0)) / 10.0)
        except OverflowError:
            return math.inf


def hop_frames(sample_rate):
    """The frames of a hop, a tenth of a second: floor(rate / 10 + 1/2)"""
    return int(math.floor(sample_rate / 10.0 + 0.5))


def kweight(sample_rate):
    """BS.1770's K-weighting at sample_rate as two sections (b0, b1, b2, a1, a2), float64 [2, 5]: the shelf, then the
    high-pass.  ValueError: a rate that is not finite, below 160 Hz (a hop is at least 16 frames) or not above 3000 Hz (the
    shelf's 1500 Hz has to lie below the Nyquist frequency)."""
    rate = _f32_finite("sample_rate", sample_rate)
    if hop_frames(rate) < MIN_HOP:
        raise ValueError(f"loudness at {sample_rate} Hz: a hop of a tenth of a second has to be at least {MIN_HOP} frames")
    if not rate > 3000.0:
        raise ValueError(f"loudness at {sample_rate} Hz: the K-weighting's shelf at 1500 Hz needs a rate above 3000 Hz")
    return np.stack([highshelf(rate, 1500.0, math.sqrt(0.5), 4.0), highpass(rate, 38.0, 0.5)])


# ---- the specification and the twin --------------------------------------------------------------------------------------------
def _host_args(x, spec, sample_rate, lengths):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 3 or x.shape[1] == 0:
        raise ValueError(f"x must be float32 [B, C, T], not {x.dtype} {x.shape}")
    if not isinstance(spec, Level):
        raise ValueError(f"spec must be a Level, not {spec!r}")
    B, C, T = x.shape
    hop, q = 1, None
    if spec.mode == "lufs":
        if C > MAX_CHANNELS:
            raise ValueError(f"{C} channels: BS.1770 weighs at most {MAX_CHANNELS}")
        q = kweight(sample_rate)
        hop = hop_frames(float(sample_rate))
    return x, _lengths_host("lengths", lengths, B, T), hop, q


def _seq_sum(a):
    """((0 + a[0]) + a[1]) + ... of a float64 vector"""
    return np.add.accumulate(a)[-1] if len(a) else np.float64(0.0)


def _tree64(q):
    """q [..., 2^k] float64 added over its last axis as a tree of halves: q[j] += q[j + h] for h = 2^(k-1) .. 1"""
    h = q.shape[-1] // 2
    while h >= 1:
        q = q[..., :h] + q[..., h:2 * h]
        h //= 2
    return q[..., 0]


def _peak(X):
    return np.float64(np.nan) if np.isnan(X).any() else np.abs(X).max(initial=0.0)


def _gain(spec, C, v, hop, P, S, s):
    """(g, E, measured) of a row from its peak P, its sum of squares S and its hop sums s [C, nh], in the order of the apply
    launch (the module docstring); every number a numpy float64, so that IEEE's special cases are IEEE's"""
    f64 = np.float64
    A, E, g = f64(spec.linear), f64(0.0), f64(1.0)
    measured = bool(v != 0 and P != 0)
    if measured:
        if spec.mode == "lufs":
            nh = v // hop
            nb = nh - 3 if nh >= 4 else 0
            n1 = 0
            if nb:
                z = ((s[:, 0:nb] + s[:, 1:nb + 1]) + (s[:, 2:nb + 2] + s[:, 3:nb + 3])) / f64(4 * hop)
                e = f64(WEIGHTS[0]) * z[0]
                for c in range(1, C):
                    e = e + f64(WEIGHTS[c]) * z[c]
                above = e > GATE_ABS
                n1 = int(above.sum())
            measured = n1 != 0
            if measured:
                thr = f64(GATE_REL) * (_seq_sum(e[above]) / f64(n1))
                both = above & (e > thr)
                E = _seq_sum(e[both]) / f64(int(both.sum()))
        else:
            E = S / f64(C * v)
        measured = measured and bool(E != 0)
    if measured:
        g = A / P if spec.mode == "peak" else np.sqrt(A / E)
        if spec.max_peak is not None:
            most = f64(spec.max_peak) / P
            if most < g:
                g = most
    return f64(g), f64(E), measured


def _twin_sum_squares(X):
    """The measure launch's sum of the squares of X float64 [n] (a plane's valid frames), in its order"""
    n = X.shape[0]
    tiles = -(-n // TILE)
    sq = np.zeros(tiles * TILE)
    sq[:n] = X * X
    sq = sq.reshape(tiles, THREADS // _LANES, _LANES, CHUNK)
    lane = np.zeros(sq.shape[:3])
    for j in range(CHUNK):
        lane = lane + sq[..., j]
    return _seq_sum(_tree64(_tree64(lane)))


def _twin_hop_sums(W, hop):
    """The measure launch's hop sums of the weighted planes W float64 [R, n], in its order: [R, n // hop]"""
    R, n = W.shape
    nh = n // hop
    if nh == 0:
        return np.zeros((R, 0))
    k = np.arange(nh)[:, None, None]
    slots = (hop + CHUNK - 2) // CHUNK + 1                           # the most chunks a hop touches
    chunk = k * hop // CHUNK + np.arange(slots)[None, :, None]
    frame = CHUNK * chunk + np.arange(CHUNK)[None, None, :]          # [nh, slots, CHUNK]
    inside = (frame >= k * hop) & (frame < (k + 1) * hop)
    sq = W * W
    vals = np.where(inside[None], sq[:, np.minimum(frame, n - 1)], 0.0)
    part = np.zeros(vals.shape[:3])
    for j in range(CHUNK):
        part = part + vals[..., j]
    return np.add.accumulate(part, axis=2)[..., -1]


def _measure(x, v, hop, q, twin):
    """(P [B], S [B], s: a list of [C, nh_b] or None) of every row, by the specification's arithmetic or the twin's"""
    B, C, T = x.shape
    P, S, s = np.zeros(B), np.zeros(B), [None] * B
    with np.errstate(all="ignore"):
        for b in range(B):
            X = x[b, :, :int(v[b])].astype(np.float64)
            P[b] = _peak(X)
            if twin:
                for c in range(C):
                    t = _twin_sum_squares(X[c])
                    S[b] = S[b] + t if c else t
            else:
                S[b] = (X * X).sum()
        if q is not None:
            for length in np.unique(v[v >= 4 * hop]):      # the rows of one length together: the loop over the samples is Python's
                rows = np.nonzero(v == length)[0]
                n, R = int(length), len(rows)
                X = x[rows, :, :n].astype(np.float64)
                if twin:
                    W = _twin_rows(X.reshape(R * C, n), np.broadcast_to(q, (R * C, 2, 5)), np.ones(R * C))
                    hops = _twin_hop_sums(W, hop).reshape(R, C, -1)
                else:
                    W = _sequential(X, np.broadcast_to(q, (R, 2, 5)))[0]
                    nh = n // hop
                    hops = (W[:, :, :nh * hop] ** 2).reshape(R, C, nh, hop).sum(axis=3)
                for i, b in enumerate(rows):
                    s[b] = hops[i]
    return P, S, s


def _level_rows(x, spec, sample_rate, lengths, twin):
    x, v, hop, q = _host_args(x, spec, sample_rate, lengths)
    B, C, T = x.shape
    P, S, s = _measure(x, v, hop, q, twin)
    g, E, live = np.ones(B), np.zeros(B), np.zeros(B, dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            g[b], E[b], measured = _gain(spec, C, int(v[b]), hop, P[b], S[b], s[b] if s[b] is not None else np.zeros((C, 0)))
            live[b] = measured and (g[b] != 1.0 or spec.clamp)
    return x, v, g, E, P, live


def level_host(x, spec, sample_rate=None, lengths=None, details=False):
    """The specification in numpy: x float32 [B, C, T], spec a `Level`, sample_rate the rate of x (lufs needs it), lengths [B]
    integers (default T) to s float64 [B, C, T]: g x, unrounded, with `clamp` limited to -1 .. 1; x itself behind the lengths
    and in the rows that are not written.  details=True: returns (s, g, E, P), float64 [B] each."""
    x, v, g, E, P, live = _level_rows(x, spec, sample_rate, lengths, twin=False)
    s = x.astype(np.float64)
    with np.errstate(all="ignore"):
        for b in np.nonzero(live)[0]:
            y = g[b] * s[b, :, :v[b]]
            if spec.clamp:
                y = np.where(np.isnan(y), y, np.minimum(np.maximum(y, -1.0), 1.0))
            s[b, :, :v[b]] = y
    return (s, g, E, P) if details else s


def level_host_twin(x, spec, sample_rate=None, lengths=None, details=False):
    """The kernel's arithmetic in numpy, its blocking and the order of its sums operation by operation with nothing fused (the
    module docstring): x float32 [B, C, T] to float32 [B, C, T]; details=True: (y, g, E, P).  The kernel equals it bit for bit."""
    x, v, g, E, P, live = _level_rows(x, spec, sample_rate, lengths, twin=True)
    y = x.copy()
    with np.errstate(all="ignore"):
        for b in np.nonzero(live)[0]:
            r = (g[b] * x[b, :, :v[b]].astype(np.float64)).astype(np.float32)
            if spec.clamp:
                r = np.where(np.isnan(r), r, np.minimum(np.maximum(r, np.float32(-1)), np.float32(1)))
            y[b, :, :v[b]] = r
    return (y, g, E, P) if details else y


def loudness_host(x, sample_rate, lengths=None, twin=False):
    """The BS.1770-4 integrated loudness of every row of x float32 [B, C, T] at sample_rate: -0.691 + 10 log10(E), float64
    [B]; -inf where nothing passes the gate.  twin=True: by the kernel's blocked arithmetic, which long rows want -- the
    sequential recurrence is a Python loop over the samples."""
    E = _level_rows(x, Level.lufs(), sample_rate, lengths, twin=twin)[3]
    with np.errstate(all="ignore"):
        return -_OFFSET + 10.0 * np.log10(E)


# ---- on the device -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _kweight_device(sample_rate, device):
    """kweight(sample_rate) as a float64 tensor [2, 5] on `device`, made once"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(kweight(sample_rate))).to(device)


def _checked(spec, sample_rate, channels):
    """The first check of `_level` and of `Corpus.crops(level=)`, without a device: (mode, hop) of a Level for crops of
    `channels` channels at sample_rate; ValueError otherwise"""
    if not isinstance(spec, Level):
        raise ValueError(f"level must be a level.Level, not {spec!r}")
    if spec.mode != "lufs":
        return spec.code, 1
    if channels > MAX_CHANNELS:
        raise ValueError(f"{channels} channels: BS.1770 weighs at most {MAX_CHANNELS}")
    if sample_rate is None:
        raise ValueError("loudness needs the sample rate of the crops")
    kweight(sample_rate)
    return spec.code, hop_frames(float(sample_rate))


def _level(ctx, x, spec, sample_rate, lengths, out):
    """`level` behind its first check; ctx() gives the context that runs it (the corpus's own inside `Corpus.crops`)"""
    import torch

    stride = _planes("x", x)
    B, C, T = x.shape
    mode, hop = _checked(spec, sample_rate, C)
    if out is not None and out is not x and (
            not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
            or (x.numel() and (_lines(out) is None or _lines(out)[0] != stride))):
        raise ValueError("out must be x itself or a float32 tensor of x's shape, layout and device")
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    d_valid = _lengths_device("lengths", lengths, B, x.device)
    if out is None:
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        if x.numel():
            out.copy_(x)        # (what the kernel leaves untouched is x's)
    if x.numel() == 0:
        return out
    q = _kweight_device(float(sample_rate), str(x.device)) if mode == LUFS else None
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ctx().level_device(x, out, B, C, stride, T, d_valid, mode, hop, q, spec.linear, spec.max_peak or 0.0, spec.clamp, None, None,
                           None, stream=stream)
    return out


def level(x, spec, sample_rate=None, lengths=None, out=None):
    """Every row of a batch brought to the level of spec, a `Level`, on the GPU: x float32 [B, C, T] on the device, contiguous
    or the slice [..., :T] of a contiguous tensor (what lies behind the slice is neither read nor written).  sample_rate: the
    rate of x, which lufs needs.  lengths: [B] integers, a sequence or a tensor (as `crops` returns them; -1 counts as 0, more
    than T as T): the frames of a row that are measured and scaled.  out: x itself (in place) or a tensor of x's shape and
    layout apart from it, of which the frames behind the lengths and the rows with nothing to measure are left as they are;
    default: a new copy of x.  Returns out.  Two launches, asynchronous on the current stream, nothing read back; ValueError
    before any device work: a spec that is no Level, and for lufs more than 5 channels or a rate that is missing, below 160 Hz
    or not above 3000 Hz."""
    ctx = _device_context("x", x, "[B, C, T]")
    return _level(ctx, x, spec, sample_rate, lengths, out)


def loudness(x, sample_rate, lengths=None):
    """The BS.1770-4 integrated loudness of every row of x (as for `level`) in LUFS: a float64 device tensor [B], -inf where
    nothing passes the gate.  The measure launch and the combination of `level` with nothing written to x; the decibels are
    torch's.  Nothing is read back."""
    import torch

    ctx = _device_context("x", x, "[B, C, T]")
    stride = _planes("x", x)
    B, C, T = x.shape
    mode, hop = _checked(Level.lufs(), sample_rate, C)
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    d_valid = _lengths_device("lengths", lengths, B, x.device)
    E = torch.zeros(B, dtype=torch.float64, device=x.device)
    if x.numel():
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device).cuda_stream
            ctx().level_device(x, None, B, C, stride, T, d_valid, mode, hop, _kweight_device(float(sample_rate), str(x.device)), 1.0, 0.0,
                               False, None, E, None, stream=stream)
    return -_OFFSET + 10.0 * torch.log10(E)
