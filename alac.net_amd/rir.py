"""Simulated room impulse responses of shoebox rooms by the image-source method (alacgpu_rir_shoebox_device,
csrc/alac_rir.hip): what `Reverb` convolves a crop with when there is no corpus of recorded responses.

A row's inputs: geometry float64 [9] = room L = (Lx, Ly, Lz), source s, microphone r, in metres; beta float32 [6] =
(beta[x][0], beta[x][1], beta[y][0], ...), the reflection coefficient of the wall at 0 and of the wall at L_a of axis a; for
the call: the rate fs, the frames K, an odd filter length W = 2 H + 1 in 3 .. MAX_TAPS, the sound speed c, max_order or None.

Image (n, p), n in Z^3, p in {0, 1}^3:

    x_a   = (1 - 2 p_a) s_a + 2 n_a L_a - r_a              the coordinate on axis a
    d     = sqrt(x_x^2 + x_y^2 + x_z^2),   tau = d fs / c   distance and delay in samples
    order = sum over a of |2 n_a - p_a|
    A     = prod over a of beta[a][0]^|n_a - p_a| * beta[a][1]^|n_a| / (4 pi d)

    h[k] = sum over the images with |t| < W / 2, t = k - tau, of A * 0.5 (1 + cos(2 pi t / W)) * sinc(t)      0 <= k < K

in ascending (nx, ny, nz, p), p counted as 4 px + 2 py + pz; only images of order <= max_order where that is given; taps
below 0 and at or above K are dropped.  rir_length is K for every row that is computed -- also where the room is so large
that no image arrives below K and the row is all zeros: `reverb` then finds an energy of 0 and leaves the crop alone.

A row is refused -- all zeros, rir_length 0, which `reverb` leaves alone bit for bit -- where one of the nine numbers is not
finite, a dimension is not positive, a coordinate of s or r lies outside 0 .. L_a, or the candidate box holds more than
LIMIT images.  The box: with dmax = (K + W) / (fs / c), N_a = floor(dmax / (2 L_a)) + 2 (|x_a| >= 2 L_a (|n_a| - 1), so no
image outside |n_a| < N_a reaches a tap below K), with max_order N_a = min(N_a, (max_order + 1) div 2); the box holds
8 (2 Nx + 1)(2 Ny + 1)(2 Nz + 1) candidates; a quotient dmax / (2 L_a) of 2^20 or more refuses the row at once.  The limit
keeps a room of a millimetre from occupying the device for minutes; a 3 x 3 x 2.5 m room at 0.5 s and 16 kHz has 2.2e6
candidates, the smallest room of Ko et al.'s "small" range (1 x 1 x 2 m) 2.3e7.  An image at d == 0 (source and microphone at
one point) gives an infinity, or a NaN with a beta of 0: it is not hidden, and `reverb`'s rule for an energy that is not
finite leaves that crop alone.

The kernel's order (csrc/alac_rir.h), which `rir_host_f32` follows operation for operation.  In float64, each operation
rounded once, per image:  x_a = ((1 - 2 p_a) s_a + (2 n_a) L_a) - r_a;  d = sqrt((xx xx + xy xy) + xz xz);  tau = d scale,
scale = fs / c;  k0 = floor(tau + 0.5);  f = tau - k0 (in -0.5 .. 0.5).  A float32 distance of 170 m is wrong by 7e-4
samples; in float64 nothing of this matters (ten operations an image).  In float32, each operation rounded once, none fused,
no library function:

    ff = float32(f);  x = PI ff;  sp = sin_poly(x);  phi = TW ff, TW = float32(2 pi / W);  cphi = cos_poly(phi);  sphi = sin_poly(phi)
    sin_poly(x) = x + (x z) q,  z = x x,  q = ((((S6 z + S5) z + S4) z + S3) z + S2) z + S1      S_i = (-1)^i / (2 i + 1)!
    cos_poly(x) = 1 + z q,               q = ((((C6 z + C5) z + C4) z + C3) z + C2) z + C1      C_i = (-1)^i / (2 i)!
    pow(b, e):  r = 1;  while e: (if e odd: r = r b);  b = b b;  e = e div 2                 the recurrence of the powers
    g = ((pow(bx0, |nx - px|) pow(bx1, |nx|)) (pow(by0, |ny - py|) pow(by1, |ny|))) (pow(bz0, |nz - pz|) pow(bz1, |nz|))
    A = g / float32(4 pi d)                                   the product 4 pi d in float64, the division correctly rounded

and per tap k = k0 + m, -H <= m <= H, 0 <= k < K, with the table (cw, sw)[j] = float32(cos, sin)(2 pi j / W), j <= H,
computed in float64:

    c = cw[|m|] cphi + (sign m) sw[|m|] sphi;   w = 0.5 + 0.5 c              the angle addition: cos(2 pi (m - f) / W)
    tt = float32(m) - ff;   s = 1 where tt == 0, else (sp for odd m, -sp for even m) / (PI tt)          sin(pi (m - f)) = -(-1)^m sin(pi f)
    h[k] = h[k] + A (w s)

(|t| < W / 2 is |m| <= H, up to a tap at |t| = W / 2 exactly, where the window is 0.)  A tap's additions run over the images
in the stated order, from 0; the tiling changes no bit.

The bound, derived, not measured.  u = 2^-24, gamma_k = k u / (1 - k u).  ff = f (1 + u); x = pi f within 3 u relative (PI, ff,
the product), so sin(x) within 3 u x / sin x <= 4.8 u; the polynomial's truncation is below x^15 / 15! <= 6.7e-10 for
|x| <= pi / 2 and its Horner evaluation within gamma_14 sinh(x) / x <= 21 u of sin(x) / x >= 0.63: sp = sin(pi f)(1 + 40 u).
tt = t (1 + 2 u) for |m| >= 1 (|t| >= 0.5) and -ff exactly for m = 0; PI, the product and the division add 3 u:
s' = s (1 + 48 u).  The window: |phi| <= pi / 3 + , the table within u / 2, cphi and sphi within 8 u absolutely (argument 3 u,
truncation below 3e-11, evaluation gamma_12 cosh(1.05)), two products, a sum, a product and a sum: |w' - w| <= 16 u.  A power
by the recurrence is within gamma_(e - 1) of b^e (the squares carry 2^i - 1 roundings into a factor of weight 2^i), the
six of them, their five products, float32(4 pi d) and the division within gamma_(R + 8), R the sum of the six exponents.
The float64 part is off by at most dtau = 8 * 2^-53 tau samples, and |d/dt (w sinc)| < 3.  So a term v = A w s is computed
within

    e = |A| ((|w| + 16 u)(|s| (1 + 48 u))(1 + gamma_(R + 10)) - |w| |s| + 3 dtau)

and the n_k float32 additions of tap k add gamma_(n_k) sum (|v| + e):  dH[k] = sum e + gamma_(n_k) sum (|v| + e).
`rir_host(..., bound=True)` returns it; it assumes that nothing underflows and that no d is 0.

`ShoeboxRooms`, `rir_host`, `rir_host_f32` and `image_counts` need no device.  `simulate_rir` is the call on device tensors;
`Reverb(ShoeboxRooms(...))` puts it behind `Corpus.crops(reverb=)`.
"""
import math

import numpy as np

from ._stageargs import _f32_finite, _Spec

_U = 2.0 ** -24
# csrc/alac_rir.h
TILE = 64
MAX_TAPS = 127
MAX_FRAMES = 1 << 20
LIMIT = 1 << 25
_PI64 = 3.14159265358979323846
_FOUR_PI = 4.0 * _PI64
_PI = np.float32(3.14159274)
_S = tuple(np.float32(v) for v in (-1.66666672e-1, 8.33333377e-3, -1.98412701e-4, 2.75573188e-6, -2.50521079e-8, 1.6059044e-10))
_C = tuple(np.float32(v) for v in (-5.0e-1, 4.16666679e-2, -1.38888892e-3, 2.48015876e-5, -2.75573203e-7, 2.08767559e-9))


def window_table(taps):
    """The kernel's table: (cos, sin)(2 pi j / W), j <= H, computed in float64 and rounded once to float32, and TW"""
    a = 2.0 * _PI64 * np.arange(taps // 2 + 1, dtype=np.float64) / float(taps)
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32), np.float32(2.0 * _PI64 / float(taps))


def _call_args(sample_rate, frames, taps, max_order, sound_speed):
    """The call's scalars, checked as `simulate_rir` and the C ABI check them; returns (fs, K, W, max_order or -1, c)"""
    for name, v in (("sample_rate", sample_rate), ("frames", frames), ("taps", taps)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, not {v!r}")
    if not 1 <= sample_rate <= 0x7FFFFFFF:
        raise ValueError(f"sample_rate must be positive, not {sample_rate!r}")
    if not 1 <= frames <= MAX_FRAMES:
        raise ValueError(f"frames must be in 1 .. {MAX_FRAMES}, not {frames!r}")
    if not 3 <= taps <= MAX_TAPS or taps % 2 == 0:
        raise ValueError(f"taps must be odd and in 3 .. {MAX_TAPS}, not {taps!r}")
    if max_order is not None and (isinstance(max_order, (bool, np.bool_)) or not isinstance(max_order, (int, np.integer))
                                  or not 0 <= max_order <= 0x7FFFFFFF):
        raise ValueError(f"max_order must be None or an integer that is not negative, not {max_order!r}")
    c = _f32_finite("sound_speed", sound_speed)
    if not c > 0.0:
        raise ValueError(f"sound_speed must be positive, not {sound_speed!r}")
    return int(sample_rate), int(frames), int(taps), -1 if max_order is None else int(max_order), c


def _host_args(geometry, beta):
    geometry, beta = np.asarray(geometry), np.asarray(beta)
    if geometry.dtype != np.float64 or geometry.ndim != 2 or geometry.shape[1] != 9:
        raise ValueError(f"geometry must be float64 [B, 9], not {geometry.dtype} {geometry.shape}")
    if beta.dtype != np.float32 or beta.shape != (geometry.shape[0], 6):
        raise ValueError(f"beta must be float32 [{geometry.shape[0]}, 6], not {beta.dtype} {beta.shape}")
    return geometry, beta


def candidate_box(geom, scale, K, H, max_order):
    """(Nx, Ny, Nz) of a row's candidate box, or None where the row is refused (the module docstring): the decision the
    kernel makes, in its float64 operations"""
    geom = np.asarray(geom, dtype=np.float64)
    if not np.all(np.isfinite(geom)):
        return None
    L, s, r = geom[0:3], geom[3:6], geom[6:9]
    if not (np.all(L > 0.0) and np.all(s >= 0.0) and np.all(s <= L) and np.all(r >= 0.0) and np.all(r <= L)):
        return None
    dmax = float(K + H + H + 1) / scale
    N, count = [], 8.0
    for a in range(3):
        q = dmax / (L[a] + L[a])
        if not q < 1048576.0:
            return None
        n = int(q) + 2
        if max_order >= 0:
            n = min(n, (max_order + 1) // 2)
        N.append(n)
        count *= float(2 * n + 1)
    return None if count > float(LIMIT) else tuple(N)


def box_candidates(room, seconds, sound_speed=343.0):
    """The candidates of a room's box for a response of `seconds`, without the filter's half length (which needs a rate):
    what `Reverb` holds a policy's smallest room to"""
    dmax = float(seconds) * float(sound_speed)
    count = 8.0
    for L in room:
        count *= 2.0 * (math.floor(dmax / (2.0 * float(L))) + 2.0) + 1.0
    return count


def _images(geom, scale, K, H, max_order, N, last=None):
    """The images of a row that reach a tap below K (at or below `last`, where given), in the stated order: (n [M, 3], p [M, 3], d, tau, k0 int64, f), the
    float64 part in the kernel's operations"""
    Nx, Ny, Nz = N
    ax = [np.arange(-n, n + 1, dtype=np.int64) for n in (Nx, Ny, Nz)] + [np.arange(8, dtype=np.int64)]
    nx, ny, nz, pi = (g.reshape(-1) for g in np.meshgrid(*ax, indexing="ij"))
    n = np.stack([nx, ny, nz], axis=1)
    p = np.stack([pi >> 2, (pi >> 1) & 1, pi & 1], axis=1)
    L, s, r = geom[0:3], geom[3:6], geom[6:9]
    x = ((1 - 2 * p).astype(np.float64) * s + (2 * n).astype(np.float64) * L) - r
    d = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    tau = d * scale
    kf = np.floor(tau + 0.5)
    f = tau - kf
    keep = kf - float(H) <= float(K - 1 if last is None else last)
    if max_order >= 0:
        keep &= np.abs(2 * n - p).sum(axis=1) <= max_order
    return n[keep], p[keep], d[keep], tau[keep], kf[keep].astype(np.int64), f[keep]


def image_counts(geometry, sample_rate, frames, taps=81, max_order=None, sound_speed=343.0):
    """(images whose window of `taps` begins below `frames`: tau - taps / 2 < frames, candidates of the box) of one row
    geometry float64 [9]; (0, 0) for a row that is refused"""
    fs, K, W, mo, c = _call_args(sample_rate, frames, taps, max_order, sound_speed)
    geom = np.asarray(geometry, dtype=np.float64).reshape(9)
    N = candidate_box(geom, float(fs) / c, K, W // 2, mo)
    if N is None:
        return 0, 0
    return len(_images(geom, float(fs) / c, K, W // 2, mo, N, last=K)[2]), 8 * (2 * N[0] + 1) * (2 * N[1] + 1) * (2 * N[2] + 1)


def _exponents(n, p):
    """[M, 6]: |n_a - p_a| and |n_a| per axis, in beta's order"""
    e = np.empty((n.shape[0], 6), dtype=np.int64)
    e[:, 0::2] = np.abs(n - p)
    e[:, 1::2] = np.abs(n)
    return e


def rir_host(geometry, beta, sample_rate, frames, taps=81, max_order=None, sound_speed=343.0, bound=False):
    """The specification in numpy float64: geometry float64 [B, 9], beta float32 [B, 6] to (h float64 [B, 1, K], rir_lengths
    int32 [B]).  bound=True: (h, rir_lengths, dH), dH float64 like h: how far a float32 evaluation in the kernel's order may
    be from h (the module docstring)."""
    geometry, beta = _host_args(geometry, beta)
    fs, K, W, mo, c = _call_args(sample_rate, frames, taps, max_order, sound_speed)
    B, H, scale = geometry.shape[0], W // 2, float(fs) / c
    h = np.zeros((B, 1, K))
    dH = np.zeros((B, 1, K))
    lengths = np.zeros(B, dtype=np.int32)
    gam = lambda k: k * _U / (1 - k * _U)
    m = np.arange(-H, H + 1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            N = candidate_box(geometry[b], scale, K, H, mo)
            if N is None:
                continue
            lengths[b] = K
            n, p, d, tau, k0, _ = _images(geometry[b], scale, K, H, mo, N)
            e = _exponents(n, p)
            A = np.prod(beta[b].astype(np.float64)[None, :] ** e, axis=1) / (_FOUR_PI * d)
            R = e.sum(axis=1)
            count, total = np.zeros(K), np.zeros(K)
            for lo in range(0, len(d), 1 << 16):
                sl = slice(lo, lo + (1 << 16))
                k = k0[sl, None] + m[None, :]
                t = k.astype(np.float64) - tau[sl, None]
                inside = np.abs(t) < W / 2.0
                w = np.where(inside, 0.5 * (1.0 + np.cos(2.0 * np.pi * t / W)), 0.0)
                s = np.sinc(t)
                v = A[sl, None] * w * s
                ok = (k >= 0) & (k < K)
                h[b, 0] += np.bincount(k[ok], weights=v[ok], minlength=K)
                if bound:
                    aw, as_ = np.abs(w), np.abs(s)
                    err = np.abs(A[sl, None]) * ((aw + 16 * _U) * (as_ * (1 + 48 * _U)) * (1 + gam(R[sl, None] + 10)) - aw * as_
                                                 + 3 * 8 * 2.0 ** -53 * tau[sl, None])
                    dH[b, 0] += np.bincount(k[ok], weights=err[ok], minlength=K)
                    count += np.bincount(k[ok], minlength=K)
                    total += np.bincount(k[ok], weights=(np.abs(v) + err)[ok], minlength=K)
            dH[b, 0] += gam(count) * total
    return (h, lengths, dH) if bound else (h, lengths)


def _sin_poly(x):
    z = x * x
    q = _S[5]
    for c in _S[4::-1]:
        q = q * z + c
    return x + (x * z) * q


def _cos_poly(x):
    z = x * x
    q = _C[5]
    for c in _C[4::-1]:
        q = q * z + c
    return np.float32(1) + z * q


def _pow_f32(b, e):
    """The kernel's recurrence, on float32 b and integer e arrays of one shape"""
    b = b.copy()
    e = e.copy()
    r = np.ones(b.shape, dtype=np.float32)
    while e.any():
        r = np.where(e & 1, r * b, r)
        b = b * b
        e >>= 1
    return r


def rir_host_f32(geometry, beta, sample_rate, frames, taps=81, max_order=None, sound_speed=343.0):
    """The kernel's order in numpy, one operation at a time (the module docstring): geometry float64 [B, 9], beta float32
    [B, 6] to (h float32 [B, 1, K], rir_lengths int32 [B]).  The kernel equals it bit for bit."""
    geometry, beta = _host_args(geometry, beta)
    fs, K, W, mo, c = _call_args(sample_rate, frames, taps, max_order, sound_speed)
    B, H, scale = geometry.shape[0], W // 2, float(fs) / c
    f32 = np.float32
    h = np.zeros((B, 1, K), dtype=f32)
    lengths = np.zeros(B, dtype=np.int32)
    cw, sw, TW = window_table(W)
    m = np.arange(-H, H + 1, dtype=np.int64)
    cwm, swm = cw[np.abs(m)], np.where(m < 0, -sw[np.abs(m)], sw[np.abs(m)]).astype(f32)
    odd = (m & 1).astype(bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            N = candidate_box(geometry[b], scale, K, H, mo)
            if N is None:
                continue
            lengths[b] = K
            n, p, d, tau, k0, f = _images(geometry[b], scale, K, H, mo, N)
            e = _exponents(n, p)
            pw = _pow_f32(np.broadcast_to(beta[b][None, :], e.shape).astype(f32), e)
            g = ((pw[:, 0] * pw[:, 1]) * (pw[:, 2] * pw[:, 3])) * (pw[:, 4] * pw[:, 5])
            A = g / (_FOUR_PI * d).astype(f32)
            ff = f.astype(f32)
            sp = _sin_poly(_PI * ff)
            phi = TW * ff
            cphi, sphi = _cos_poly(phi), _sin_poly(phi)
            row = h[b, 0]
            for lo in range(0, len(d), 1 << 16):
                sl = slice(lo, lo + (1 << 16))
                cc = cwm[None, :] * cphi[sl, None] + swm[None, :] * sphi[sl, None]
                w = f32(0.5) + f32(0.5) * cc
                tt = m.astype(f32)[None, :] - ff[sl, None]
                num = np.where(odd[None, :], sp[sl, None], -sp[sl, None])
                s = np.where(tt == 0, f32(1), num / (_PI * tt)).astype(f32)
                v = A[sl, None] * (w * s)
                k = k0[sl, None] + m[None, :]
                ok = (k >= 0) & (k < K)
                np.add.at(row, k[ok], v[ok])                # in the order given: image-major, so ascending images a tap
    return h, lengths


# ---- the rooms -------------------------------------------------------------------------------------------------------------------
def _range(name, v, least):
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise ValueError(f"{name} must be a pair (low, high), not {v!r}")
    lo, hi = _f32_finite(name, v[0]), _f32_finite(name, v[1])
    if not least < lo <= hi:
        raise ValueError(f"{name} must be a pair {least} < low <= high, not {v!r}")
    return lo, hi


_KALDI = dict(small=((1.0, 10.0), (1.0, 10.0), (2.0, 5.0)), medium=((10.0, 30.0), (10.0, 30.0), (2.0, 5.0)),
              large=((30.0, 50.0), (30.0, 50.0), (2.0, 5.0)))


class ShoeboxRooms(_Spec):
    """A policy of shoebox rooms for `Reverb`: every crop gets a room, a source and a microphone of its own.  room: three
    ranges (low, high) in metres, drawn uniformly.  absorption: a range of the walls' absorption alpha within 0 .. 1, drawn
    uniformly, beta = sqrt(1 - alpha) for the six walls; or rt60: a range in seconds, from which Sabine's
    alpha = 0.161 V / (S rt60), clipped to 0.01 .. 0.99.  Exactly one of the two (absorption=None with rt60).  margin: the
    source and the microphone are each uniform in the room less `margin` metres at every wall; 2 margin may not exceed the
    smallest dimension.  taps, max_order, sound_speed: as `simulate_rir`.  Immutable.  ValueError otherwise."""

    __slots__ = ("room", "absorption", "rt60", "margin", "taps", "max_order", "sound_speed")

    def __init__(self, room=((3, 10), (3, 10), (2.5, 4)), absorption=(0.2, 0.8), rt60=None, margin=0.5, taps=81, max_order=None,
                 sound_speed=343.0):
        s = object.__setattr__
        if not isinstance(room, (tuple, list)) or len(room) != 3:
            raise ValueError(f"room must be three ranges (low, high), not {room!r}")
        room = tuple(_range("a range of room", r, 0.0) for r in room)
        if (absorption is None) == (rt60 is None):
            raise ValueError("exactly one of absorption and rt60 is given")
        if absorption is not None:
            absorption = _range("absorption", absorption, -1.0)
            if not (0.0 <= absorption[0] and absorption[1] <= 1.0):
                raise ValueError(f"absorption must be within 0 .. 1, not {absorption!r}")
        else:
            rt60 = _range("rt60", rt60, 0.0)
        margin = _f32_finite("margin", margin, 0.0)
        if 2.0 * margin > min(r[0] for r in room):
            raise ValueError(f"twice the margin {margin!r} exceeds the smallest dimension of room {room!r}")
        _, _, taps, mo, c = _call_args(1, 1, taps, max_order, sound_speed)
        for k, v in (("room", room), ("absorption", absorption), ("rt60", rt60), ("margin", margin), ("taps", taps),
                     ("max_order", None if mo < 0 else mo), ("sound_speed", c)):
            s(self, k, v)

    @classmethod
    def kaldi(cls, size, **more):
        """Ko et al. 2017's ranges: "small" rooms of 1 .. 10 m by 1 .. 10 m, "medium" 10 .. 30 m, "large" 30 .. 50 m, each
        2 .. 5 m high, absorption 0.2 .. 0.8"""
        if size not in _KALDI:
            raise ValueError(f"size must be one of {sorted(_KALDI)}, not {size!r}")
        return cls(room=_KALDI[size], absorption=(0.2, 0.8), **more)

    def smallest(self):
        return tuple(r[0] for r in self.room)

    def draw(self, batch, generator=None, device=None):
        """(geometry float64 [B, 9], beta float32 [B, 6]) on `device`.  Four draws of float64 rand, always in this order, 10 B
        values: the room [B, 3], the absorption or the rt60 [B], the source [B, 3], the microphone [B, 3]; each value is
        low + (high - low) k.  generator: a torch.Generator of `device` or of the CPU (the draws are then made there and
        uploaded); default: the device's own.  Nothing is read back."""
        import torch

        from . import _frame_count

        B = _frame_count("batch", batch)
        dev = generator.device if generator is not None else device
        rand = lambda *shape: torch.rand(*shape, generator=generator, device=dev, dtype=torch.float64)
        lo = torch.tensor([r[0] for r in self.room], dtype=torch.float64, device=dev)
        hi = torch.tensor([r[1] for r in self.room], dtype=torch.float64, device=dev)
        L = lo + (hi - lo) * rand(B, 3)
        k = rand(B)
        if self.absorption is not None:
            alpha = self.absorption[0] + (self.absorption[1] - self.absorption[0]) * k
        else:
            t = self.rt60[0] + (self.rt60[1] - self.rt60[0]) * k
            V = L[:, 0] * L[:, 1] * L[:, 2]
            S = 2.0 * (L[:, 0] * L[:, 1] + L[:, 0] * L[:, 2] + L[:, 1] * L[:, 2])
            alpha = (0.161 * V / (S * t)).clamp(0.01, 0.99)
        free = L - 2.0 * self.margin
        src = self.margin + free * rand(B, 3)
        mic = self.margin + free * rand(B, 3)
        geometry = torch.cat([L, src, mic], dim=1).contiguous()
        beta = torch.sqrt(1.0 - alpha).to(torch.float32)[:, None].expand(B, 6).contiguous()
        return geometry.to(device), beta.to(device)


# ---- on the device ---------------------------------------------------------------------------------------------------------------
def _simulate(ctx, geometry, beta, sample_rate, frames, taps, max_order, sound_speed, out):
    """`simulate_rir` behind its first check; ctx() gives the context that runs it, asked for behind the checks"""
    import torch

    fs, K, W, mo, c = _call_args(sample_rate, frames, taps, max_order, sound_speed)
    if geometry.dtype != torch.float64 or geometry.dim() != 2 or geometry.shape[1] != 9 or not geometry.is_contiguous():
        raise ValueError("geometry must be a contiguous float64 device tensor [B, 9]")
    B = geometry.shape[0]
    if (not isinstance(beta, torch.Tensor) or beta.device != geometry.device or beta.dtype != torch.float32 or beta.shape != (B, 6)
            or not beta.is_contiguous()):
        raise ValueError(f"beta must be a contiguous float32 tensor [{B}, 6] on geometry's device")
    stride = K
    if out is None:
        out = torch.empty((B, 1, K), dtype=torch.float32, device=geometry.device)
    else:
        from ._stageargs import _planes

        stride = _planes("out", out, B, K, (1,))
        if out.device != geometry.device:
            raise ValueError("out must be on geometry's device")
    lengths = torch.empty(B, dtype=torch.int32, device=geometry.device)
    if B == 0:
        return out, lengths
    with torch.cuda.device(geometry.device):
        stream = torch.cuda.current_stream(geometry.device).cuda_stream
        ctx().rir_shoebox_device(geometry, beta, B, fs, K, W, mo, c, out, stride, lengths, stream=stream)
    return out, lengths


def simulate_rir(geometry, beta, sample_rate, frames, taps=81, max_order=None, sound_speed=343.0, out=None):
    """Image-source responses of shoebox rooms on the GPU: geometry float64 [B, 9] (room, source, microphone in metres) and
    beta float32 [B, 6] (the walls' reflection coefficients: x at 0, x at Lx, y ...), contiguous on one device, to
    (rir float32 [B, 1, frames], rir_lengths int32 [B]): `frames` for a row that is computed, 0 for one that is refused and
    all zeros (the module docstring says which).  taps: the odd length of the windowed sinc, 3 .. 127.  max_order: None or
    the largest reflection order taken.  out: a float32 tensor [B, 1, frames], contiguous or the slice [..., :frames] of a
    contiguous one (what lies behind the slice is not written); default: a new one.  One launch, asynchronous on the current
    stream, nothing read back; ValueError before any device work."""
    from ._stageargs import _device_context

    return _simulate(_device_context("geometry", geometry, "[B, 9] (float64)"), geometry, beta, sample_rate, frames, taps, max_order,
                     sound_speed, out)
