"""Speed perturbation: every utterance played at a factor drawn from a few (0.9 / 1.0 / 1.1 is the standard recipe) and
resampled back to the training rate -- the resampler without tables (alacgpu_resample_ratio_rows_device, csrc/alac_resample.hip).

A signal of `rate` Hz played at the factor p / q is taken to be at rate * p / q Hz (torchaudio's SpeedPerturbation) and is
resampled to new_rate: the reduced ratio a : b of rate * p : new_rate * q, width = resample.filter_width(a, b), and
Ty = ceil(b * T / a) frames.  The filter is resample.py's, y[j] = sum over s of h(s / a - j / b) * x[s]; the float64
specification is `speed_host`: resample.apply_table with resample._table(a, b, width), whatever the table's size.

The kernel keeps no table: 44.1 kHz at 0.9 to 16 kHz is 3969 : 1600, 1600 phases of 33 taps.  It evaluates a tap's weight
where it uses it.  With M = max(a, b), j * a = q * b + r (64-bit integers), the tap d = -width .. width of output frame j
reads x[q + d] and weighs

    n = d * b - r,   v = 99 * n / (100 * M),   w = scale * sinc(v) * cos^2(pi * v / 12)  for |v| < 6, else 0,

scale = 0.99 * min(a, b) / a: f * u of resample.py is v.  In float32 (`weights_f32` restates it, operation by operation):

    k = 99 * n, an integer; mag = |k|; mag >= 600 * M: w = 0; mag == 0: w = scale32
    ms = mag mod (200 * M) (the period of sin(pi v)); minus = ms >= 100 * M, then ms -= 100 * M; ms > 50 * M: ms = 100 * M - ms
    s = sinpi(float(ms) * inv100), negated with minus            inv100  = 1 / float(100 * M)
    c = sinpi(float(600 * M - mag) * inv1200)                    inv1200 = 1 / float(1200 * M)     (cos(pi v / 12))
    pv = (float(mag) * inv100) * PI                              PI = float32(pi)
    w = scale32 * ((s * (c * c)) / pv)                           scale32 = float(99 * min(a, b)) / float(100 * a)
    sinpi(x) = x * p(x * x), 0 <= x <= 1/2: p by Horner with six fused multiply-adds over SINPI, the Taylor coefficients
    (-1)^i pi^(2i+1) / (2i+1)! of sin(pi x) up to degree 13, rounded to float32

float() of an integer rounds to nearest even; every product and the division are rounded once, correctly; nothing else is
fused.  Both sine arguments are reduced as integers, before anything is rounded, so the sines keep their relative accuracy at
their zeros.  The taps are accumulated by fused multiply-adds in ascending d from 0, as the table kernels do (`speed_host_f32`).

The bound EPS_W on |w32 - w64| / scale, w64 the table's weight, with u = 2^-24, |sinc| <= 1, |cos| <= 1 -- every term is a
relative error of a factor of w, so their sum bounds the relative error of w and, times |w| <= scale, the absolute one:
    a sine argument: the integer's conversion 1 u, the denominator's conversion 1 u, the reciprocal 1 u, the product 1 u:   4 u,
        and sin(pi x) on 0 .. 1/2 has condition pi x / tan(pi x) <= 1
    sinpi at that argument: truncation (pi / 2)^15 / 15! / 2 < 0.01 u; the rounded coefficients and the six fused
        multiply-adds, each 1 u of a partial sum, together at most 2 * sinh(pi / 2) / (sin(pi / 2) / (1 / 2)) = 2.3 times
        1 u + 1 u; x * x 1 u at condition <= 0.8; the last product 1 u:                                          < 8 u
    so s 12 u, c 12 u, c * c 25 u; pv 4 u + PI 0.5 u + its product 1 u = 5.5 u; the product s * (c * c), the division and the
    product with scale32 3 u; scale32 two conversions and a division 3 u; the table's own rounding to float32 1 u:  49.5 u,
and the second-order terms are below 0.01 u.  EPS_W = 64 u = 2^-18.  tests/test_speed_spec.py measures the worst over every
phase and tap of 9:10, 11:10, 10:9, 3969:1600, 441:160, 33:5 and 50 random reduced ratios below 4000: 8.08 u (4.82e-7).  Per
output element the kernel is then within (N + 2) * 2^-24 * sum |w x| + EPS_W * scale * sum |x| of the specification, the sums
over the element's N taps (`speed_host(..., magnitude=True)` and `speed_bound`).

`SpeedPerturb`, `ratio`, `speed_host`, `speed_host_f32`, `weights_f32` and `speed_bound` need no device.  `speed_perturb` is
the call on device tensors; `Corpus.crops(..., speed=)` runs it in front of every other stage (corpus.py).
"""
import math
from fractions import Fraction

import numpy as np

from ._stageargs import _f32_finite, _fma32, _Spec
from .resample import _ratio, _table, apply_table, filter_width, identity_table, resampled_frames

EPS_W = 2.0 ** -18
SINPI = tuple(np.float32(float.fromhex(h)) for h in ("0x1.921fb6p+1", "-0x1.4abbcep+2", "0x1.466bc6p+1", "-0x1.32d2ccp-1",
                                                     "0x1.507834p-4", "-0x1.e3075p-8", "0x1.e8f434p-12"))
PI32 = SINPI[0]
MAX_WIDTH = 20479       # a frame's own span, 2 * width + 2 floats, fits the 160 KiB of a CU: a / b up to about 3378
MAX_DENOMINATOR = 1000


def _factor(v):
    """A factor as a Fraction: an int, a Fraction, or a float read by its decimal repr (0.9 is 9 / 10)"""
    if isinstance(v, (bool, np.bool_)):
        raise ValueError(f"a factor must be an int, a Fraction or a float, not {v!r}")
    if isinstance(v, (int, np.integer)):
        f = Fraction(int(v))
    elif isinstance(v, Fraction):
        f = v
    elif isinstance(v, (float, np.floating)) and math.isfinite(float(v)):
        f = Fraction(repr(float(v)))
    else:
        raise ValueError(f"a factor must be an int, a Fraction or a float, not {v!r}")
    if not Fraction(1, 2) <= f <= 2:
        raise ValueError(f"factor {v!r} outside 1/2 .. 2")
    if f.denominator > MAX_DENOMINATOR:
        raise ValueError(f"factor {v!r} is {f}: a denominator above {MAX_DENOMINATOR}")
    return f


def ratio(rate, factor, new_rate):
    """(a, b, width) of a signal of `rate` Hz played at `factor` and resampled to new_rate: the reduced rate * p : new_rate * q
    for the factor p / q, and resample.filter_width(a, b).  T frames become ceil(b * T / a)."""
    f = _factor(factor)
    _ratio(rate, new_rate)
    a, b = _ratio(int(rate) * f.numerator, int(new_rate) * f.denominator)
    return a, b, filter_width(a, b)


class SpeedPerturb(_Spec):
    """The policy: a crop is played at one of `factors` (ints, Fractions, or floats read by their decimal repr), drawn with
    the probabilities `weights` (default: uniform), and with probability 1 - p at factor 1 whatever was drawn.  `factors` is
    the tuple the draws index: the given ones as Fractions, and 1 behind them if it is not among them; `one` is the index of
    1.  Immutable.  ValueError: a factor outside 1/2 .. 2 or with a denominator above 1000, an empty list, a duplicate,
    weights that are not as many non-negative finite numbers with a positive sum, p outside 0 .. 1."""

    __slots__ = ("factors", "weights", "p")

    def __init__(self, factors=(0.9, 1.0, 1.1), weights=None, p=1.0):
        try:
            given = tuple(_factor(v) for v in factors)
        except TypeError:
            raise ValueError(f"factors must be a sequence of factors, not {factors!r}") from None
        if not given:
            raise ValueError("factors must not be empty")
        if len(set(given)) != len(given):
            raise ValueError(f"factors {factors!r} has a duplicate")
        if weights is None:
            w = (1.0,) * len(given)
        else:
            w = tuple(_f32_finite("a weight", v, least=0.0) for v in weights)
            if len(w) != len(given) or not sum(w) > 0:
                raise ValueError(f"weights must be {len(given)} non-negative numbers with a positive sum, not {weights!r}")
        p = _f32_finite("p", p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be in 0 .. 1, not {p!r}")
        s = object.__setattr__
        s(self, "factors", given if Fraction(1) in given else given + (Fraction(1),))
        s(self, "weights", w + (0.0,) * (len(self.factors) - len(w)))
        s(self, "p", p)

    @property
    def one(self):
        return self.factors.index(Fraction(1))

    def draw(self, B, generator=None, device="cuda"):
        """Indices into `factors` for B crops: an int64 tensor [B] on `device`, by torch operations only; nothing is read
        back.  Two draws of B float64 uniforms each, in this order: u, the factor -- the first index whose cumulative weight,
        as a share of the sum, is above u --, then v: the crop keeps its factor if v < p, else it gets `one`.  generator: a
        torch.Generator of that device or of the CPU (the draws are then made there and uploaded)."""
        import torch

        here = torch.device(device)
        dev = generator.device if generator is not None else here
        cum = np.cumsum(np.asarray(self.weights, dtype=np.float64))
        edges = torch.from_numpy(cum[:-1] / cum[-1]).to(here)
        u = torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here)
        v = torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(here)
        k = torch.searchsorted(edges, u, right=True).clamp(max=len(self.factors) - 1)
        return torch.where(v < self.p, k, self.one).to(torch.int64)


# ---- the specification and its float32 twin ------------------------------------------------------------------------------------
def speed_host(x, a, b, width, mono=False, origin=0, first=0, num_frames=None, magnitude=False):
    """The specification: resample.apply_table with the table of a : b and width, float64, no limit on the table's size"""
    return apply_table(x, a, b, width, *_table(a, b, width), mono=mono, origin=origin, first=first, num_frames=num_frames,
                       magnitude=magnitude)


def speed_bound(x, a, b, width, mono=False, origin=0, first=0, num_frames=None):
    """How far the kernel may be from `speed_host`, per element: (N + 2) * 2^-24 * sum |w x| + EPS_W * scale * sum |x|, both
    sums over the element's N = 2 * width + 1 taps"""
    N = 2 * width + 1
    kw = dict(mono=mono, origin=origin, first=first, num_frames=num_frames, magnitude=True)
    d0 = _table(a, b, width)[0]
    ones = np.ones((b, N), dtype=np.float32)
    return ((N + 2) * 2.0 ** -24 * speed_host(x, a, b, width, **kw)
            + EPS_W * (0.99 * min(a, b) / a) * apply_table(x, a, b, width, d0, ones, **kw))


def _sinpi32(x):
    """sin(pi x), 0 <= x <= 1/2, as the kernel evaluates it"""
    z = x * x
    p = np.full(x.shape, SINPI[6], dtype=np.float32)
    for c in SINPI[5::-1]:
        p = _fma32(p, z, c)
    return x * p


def weights_f32(a, b, width, phases=None):
    """The kernel's weights of the ratio a : b, float32 [len(phases), 2 * width + 1]: row i is the taps d = -width .. width of
    an output frame with (j * a) mod b = phases[i] (default: every phase 0 .. b - 1) -- the module docstring's arithmetic."""
    f32 = np.float32
    M = max(a, b)
    r = np.arange(b, dtype=np.int64) if phases is None else np.asarray(phases, dtype=np.int64)
    d = np.arange(-width, width + 1, dtype=np.int64)
    k = 99 * (d[None, :] * b - r[:, None])
    mag = np.abs(k)
    ms = mag % (200 * M)
    minus = ms >= 100 * M
    ms = np.where(minus, ms - 100 * M, ms)
    ms = np.where(ms > 50 * M, 100 * M - ms, ms)
    inv100 = f32(1) / f32(100 * M)
    inv1200 = f32(1) / f32(1200 * M)
    scale = f32(99 * min(a, b)) / f32(100 * a)
    s = _sinpi32(ms.astype(f32) * inv100)
    s = np.where(minus, -s, s)
    c = _sinpi32(np.maximum(600 * M - mag, 0).astype(f32) * inv1200)
    pv = (mag.astype(f32) * inv100) * PI32
    with np.errstate(divide="ignore", invalid="ignore"):
        w = scale * ((s * (c * c)) / pv)
    w = np.where(mag == 0, scale, w)
    return np.where(mag >= 600 * M, f32(0), w).astype(f32)


def speed_host_f32(x, a, b, width, mono=False, origin=0, first=0, num_frames=None):
    """The kernel's float32 twin: x float32 [..., C, T] holds the source frames origin .. origin + T of a signal that is zero
    elsewhere; returns the target frames first .. first + num_frames (default: up to the signal's end) as float32, every
    weight by `weights_f32` and every tap one exact fused multiply-add in ascending d.  mono: (x[0] + x[1]) * 0.5 in float32
    first."""
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[-1]
    if mono and x.ndim >= 2 and x.shape[-2] == 2:
        x = (x[..., 0:1, :] + x[..., 1:2, :]) * np.float32(0.5)
    elif mono and (x.ndim < 2 or x.shape[-2] != 1):
        raise ValueError(f"mono takes [..., 1 or 2, T], not {x.shape}")
    end = resampled_frames(origin + T, a, b)
    if num_frames is None:
        num_frames = max(end - first, 0)
    N = 2 * width + 1
    j = first + np.arange(num_frames, dtype=np.int64)
    q, r = (j * a) // b, (j * a) % b
    phases, which = np.unique(r, return_inverse=True)
    w = weights_f32(a, b, width, phases)[which.reshape(-1)]                     # [n, N]
    s = (q - width)[:, None] + np.arange(N, dtype=np.int64)[None, :] - origin      # [n, N]: where in x
    inside = (s >= 0) & (s < T)
    xs = np.where(inside, x[..., np.clip(s, 0, max(T - 1, 0))] if T else np.float32(0), np.float32(0)).astype(np.float32)
    acc = np.zeros(x.shape[:-1] + (num_frames,), dtype=np.float32)
    for n in range(N):
        acc = _fma32(w[:, n], xs[..., n], acc)
    acc[..., (j < 0) | (j >= end)] = 0.0
    return acc


# ---- on the device -------------------------------------------------------------------------------------------------------------
def speed_perturb(pcm, factors, orig_rate, new_rate=None, lengths=None, mono=False):
    """Play the rows of pcm -- float32 [F, C, T] on the device, C 1 or 2, as `load_batch` returns it -- at `factors` (one
    factor, or a sequence of F) and resample them from orig_rate to new_rate (default: orig_rate), asynchronous on the
    current stream.  Returns (tensor [F, C or 1, max Ty], new lengths int64 [F] on the device): row f has
    ceil(b_f * lengths[f] / a_f) frames with its own a_f : b_f = ratio(orig_rate, factor, new_rate), zeros behind them.
    lengths: the rows' frames (a sequence or an int64 tensor, default T); what lies behind them counts as zero.  mono: the
    mean of two channels, taken in float32 in front of the filter.  A row at factor 1 with new_rate equal to orig_rate is a
    copy, bit for bit (the table that copies, through alacgpu_resample_rows_device); every other row is filtered by
    alacgpu_resample_ratio_rows_device."""
    import torch

    from .resample import _context

    if not isinstance(pcm, torch.Tensor) or pcm.device.type != "cuda" or pcm.dtype != torch.float32 or pcm.dim() != 3:
        raise ValueError("pcm must be a float32 device tensor [F, C, T]")
    F, C_, T = pcm.shape
    if C_ not in (1, 2):
        raise ValueError(f"{C_} channels: the resampler takes 1 or 2")
    new_rate = orig_rate if new_rate is None else new_rate
    many = isinstance(factors, (list, tuple, np.ndarray))
    fs = [_factor(v) for v in factors] if many else [_factor(factors)] * F
    if len(fs) != F:
        raise ValueError(f"{len(fs)} factors for {F} rows")
    dev = pcm.device
    if lengths is None:
        lens = np.full(F, T, dtype=np.int64)
    else:
        lens = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
        if lens.shape != (F,) or (F and lens.dtype.kind not in "iu"):
            raise ValueError(f"lengths must be {F} integers")
        lens = np.clip(lens.astype(np.int64), 0, T)
    index, ratios, row_ratio, copies = {}, [], [], []
    for f in fs:
        a, b, width = ratio(orig_rate, f, new_rate)
        copies.append(f == 1 and a == b)
        if width > MAX_WIDTH:
            raise ValueError(f"{orig_rate} Hz at factor {f} to {new_rate} Hz is {a} : {b}: a filter of width {width}, the kernel takes {MAX_WIDTH}")
        row_ratio.append(index.setdefault((a, b, width), len(index)))
        if len(ratios) < len(index):
            ratios.append((a, b, width))
    ratios = np.asarray(ratios, dtype=np.uint32).reshape(-1, 3)
    copies = np.asarray(copies, dtype=bool)
    ab = ratios[np.asarray(row_ratio, dtype=np.int64)].astype(np.int64) if F else np.zeros((0, 3), np.int64)
    new_lens = resampled_frames(lens, ab[:, 0], ab[:, 1]) if F else lens
    Ty = int(resampled_frames(T, ab[:, 0], ab[:, 1]).max()) if F else 0
    out = torch.empty((F, 1 if mono else C_, Ty), dtype=torch.float32, device=dev)
    d_new = torch.from_numpy(np.asarray(new_lens, dtype=np.int64)).to(dev)
    if F and Ty:
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        zeros = torch.zeros(F, dtype=torch.int64, device=dev)
        d_lens = up(lens)
        src = pcm.contiguous()
        with torch.cuda.device(dev):
            ctx, stream = _context(dev.index), torch.cuda.current_stream(dev).cuda_stream
            if copies.any():        # the rows that are copied (every other row as zeros, for the second call to fill)
                _, _, _, d0, w = identity_table()
                desc = np.array([[1, 1, 1, 0, 0]], dtype=np.uint32)
                ctx.resample_rows_device(src, F, C_, T, zeros, d_lens, zeros, Ty, desc, up(desc.view(np.int32)), up(d0), up(w.reshape(-1)),
                                         up(np.where(copies, 0, 1).astype(np.int32)), mono, out, stream=stream)
            if not copies.all():
                skip = len(ratios)
                ctx.resample_ratio_rows_device(src, F, C_, T, zeros, d_lens, zeros, Ty, ratios, up(ratios.view(np.int32)),
                                               up(np.where(copies, skip, np.asarray(row_ratio)).astype(np.int32)), mono, out, stream=stream)
    return out, d_new
