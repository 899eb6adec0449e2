"""A reference of the GPU encoder's fixed policy (the header comment of alac_encode.hip), packet by packet.

Given a packet's source samples and its stream cfg, `reference_packet` returns the packet the policy prescribes, byte for
byte, and how firm that answer is:

  * conversion: `load_sample` -- int32 clamped to the sample range; float32 scaled by 2^(ss-1) in float32, clamped, rounded
    half to even; NaN the smallest sample.  24-bit packets split the low byte off (an arithmetic >> 8) before the analysis.
  * autocorrelation over lags 0..8 in int64, frames in front of the packet taken as zero.  These sums are exact (values of at
    most 16 bits after the split, n <= 16384: every sum is below 2^44), so the GPU's float64 sums are exact in any order.
  * the seven candidates' correlations from a L + b R with the kernel's (a, b) -- A_w by this approximation, not by its
    rounded stream -- in sixteenths, exact; then r[0] *= 1 + 1e-9 in float64, as the kernel does.
  * Levinson-Durbin at order 8 in exact rational arithmetic, quantised as floor(c * 512 + 1/2), clamped to int16; all zeros
    when n <= 9 or r[0] = 0.
  * the candidates' exact bit counts from the CPU synth encoder (coef_mode 1): a weight is unusable exactly when the synth
    refuses its pair.  The smallest count over weights 0..4 wins, a tie goes to the smaller weight; the packet escapes when
    its compressed bytes are >= the escape packet's.

Firmness.  The kernel runs Levinson-Durbin in float64, with fused multiply-adds where hipcc contracts, so its c * 512 can
differ from the exact value in the last bits.  A coefficient is firm when its exact c * 512 lies further than
`delta(err64)` from a rounding boundary (a half-integer), where err64 is the largest |c * 512 - exact| of the same
candidate's plain float64 Levinson-Durbin (the same operations in the same order, without fusion).  Fusing only removes
roundings, so the GPU's error has the size of err64; delta takes 64 times it, and no less than 2^-30.  A packet is firm when
every coefficient of every candidate is; a firm packet must equal the reference byte for byte.

Measured on the test signals (test_encode_ref.py bounds it below 1e-6): the float64 error of c * 512 reaches about 1.3e-8
for pure tones, 3e-9 for the synth signals, 5e-10 for DC with silence and 1e-13 for mirrored channels; the nearest
boundary seen lies about 1e-4 away, so no packet of the suite is non-firm.
"""
from fractions import Fraction

import numpy as np

ORDER, QUANT, LAGS = 8, 9, 9
NS = 7
# candidate s = (a L + b R), a and b in quarters: 0 L, 1 R, 2..5 A_w = R + ((L - R) * w >> 2) for w = 1..4, 6 B = L - R
AB4 = [(4, 0), (0, 4), (1, 3), (2, 2), (3, 1), (4, 0), (4, -4)]
R0_BOOST = 1.0 + 1e-9
DELTA_FACTOR, DELTA_FLOOR = 64.0, 2.0 ** -30
# exact="auto": a candidate whose float64 c * 512 all lie further than GUARD from a boundary is taken as computed in float64
# (firm); GUARD is 10^4 times the largest float64 error test_encode_ref.py allows on its signals
GUARD = 1e-3


def stream_a(stereo, w):
    return 0 if not stereo else (0 if w == 0 else 1 + w)


def stream_b(w):
    return 1 if w == 0 else NS - 1


def sample_range(ss):
    return -(1 << (ss - 1)), (1 << (ss - 1)) - 1


def convert(x, ss):
    """load_sample: the canonical int64 samples of int32 or float32 input for sample size ss."""
    lo, hi = sample_range(ss)
    x = np.asarray(x)
    if x.dtype == np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            y = x * np.float32(1 << (ss - 1))          # in float32, as the kernel
            y = np.where(np.isnan(y), np.float32(lo), np.clip(y, np.float32(lo), np.float32(hi)))
        return np.rint(y).astype(np.int64)                # half to even
    assert x.dtype == np.int32, x.dtype
    return np.clip(x.astype(np.int64), lo, hi)


def autocorr(l, r):
    """Exact sums over lags 0..8 (frames before the packet are zero): l l, r r, l[i] r[i-j], r[i] l[i-j]."""
    n = len(l)
    out = np.zeros((4, LAGS), np.int64)
    for j in range(min(LAGS, n)):
        out[0, j] = np.dot(l[j:], l[:n - j])
        out[1, j] = np.dot(r[j:], r[:n - j])
        out[2, j] = np.dot(l[j:], r[:n - j])
        out[3, j] = np.dot(r[j:], l[:n - j])
    return [[int(v) for v in row] for row in out]


def candidate_r16(ac, s):
    """16 r_j of candidate s (exact integers)."""
    a, b = AB4[s]
    return [a * a * ac[0][j] + b * b * ac[1][j] + a * b * (ac[2][j] + ac[3][j]) for j in range(LAGS)]


def _levinson(r, one):
    c = [one * 0] * LAGS
    err = r[0]
    for i in range(1, ORDER + 1):
        acc = r[i]
        for j in range(1, i):
            acc -= c[j] * r[i - j]
        kk = acc / err
        tmp = list(c)
        c[i] = kk
        for j in range(1, i):
            c[j] = tmp[j] - kk * tmp[i - j]
        err *= one - kk * kk
        if not err > 0:
            break
    return c[1:]


def lpc(r16, n, exact=True):
    """(quantised coefficients, c * 512 as Fractions -- exact, or the float64 values' when exact is False --, float64
    c * 512) of one candidate; (zeros, None, None) when it has no LPC."""
    if n <= ORDER + 1 or r16[0] <= 0:
        return [0] * ORDER, None, None
    r0 = float(r16[0]) / 16.0 * R0_BOOST                 # exact r0 / 16, then the kernel's one float64 rounding
    f64 = [c * float(1 << QUANT) for c in _levinson([r0] + [v / 16.0 for v in r16[1:]], 1.0)]
    if exact:
        x = [c * (1 << QUANT) for c in _levinson([Fraction(r0)] + [Fraction(v, 16) for v in r16[1:]], Fraction(1))]
    else:
        x = [Fraction(v) for v in f64]
    q = [max(-32768, min(32767, int((v + Fraction(1, 2)).__floor__()))) for v in x]
    return q, x, f64


def boundary_distance(x):
    """How far the exact value x lies from the nearest half-integer (a rounding boundary of floor(x + 1/2))."""
    f = x - x.__floor__()
    return float(abs(f - Fraction(1, 2)))


def desc(synth, n, cfg, **kw):
    """A synth recipe for an n-frame packet of stream cfg (max_samples_per_frame, ss, pb, mb, kb, C)."""
    max_spf, ss, pb, mb, kb, C_ = cfg
    return synth.packet_descs(1, n=n, max_samples_per_frame=max_spf, sample_size=ss, stereo=int(C_ == 2),
                              rice_history_mult=pb, rice_initial_history=mb, rice_kmodifier=kb, **kw)


class Ref:
    """The reference packet of one packet, with the facts a test reports on."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def reference_packet(synth, pcm, cfg, exact=True):
    """pcm [n, C] int32 or float32 (the packet's source frames); cfg (max_samples_per_frame, ss, pb, mb, kb, C).  Returns a
    Ref: packet (bytes), samples (the canonical int64 [n, C]), weight, escape, coefs[s] (the seven candidates', or one for
    mono), nbits[w] (None: unusable), comp_bits, esc_bits, margin (escape packet bytes - compressed bytes, None when no
    weight is usable), firm, min_dist (the smallest boundary distance over the candidates' coefficients, inf: none),
    err64 (the largest float64 error of c * 512 seen).  exact="auto" runs the exact Levinson-Durbin only for candidates
    whose float64 coefficients come within GUARD of a boundary (err64 then covers those only)."""
    max_spf, ss, pb, mb, kb, C_ = cfg
    pcm = np.asarray(pcm)
    n = pcm.shape[0]
    assert pcm.shape == (n, C_) and 1 <= n <= min(max_spf, 16384)
    stereo = C_ == 2
    s = convert(pcm, ss)
    ub = 1 if ss == 24 else 0
    l = s[:, 0] >> (8 * ub)
    r = s[:, 1] >> (8 * ub) if stereo else np.zeros(n, np.int64)
    ac = autocorr(l, r)
    coefs, firm, min_dist, err64 = [], True, float("inf"), 0.0
    for sid in range(NS if stereo else 1):
        r16 = candidate_r16(ac, sid)
        q, x, f = lpc(r16, n, exact=exact is True)
        if exact == "auto" and x is not None:
            d = min(boundary_distance(v) for v in x)
            if d <= GUARD:
                q, x, f = lpc(r16, n, exact=True)
            else:
                min_dist, x = min(min_dist, d), None
        coefs.append(q)
        if x is not None:
            e = max(abs(float(xe - Fraction(fe))) for xe, fe in zip(x, f))
            err64 = max(err64, e)
            d = min(boundary_distance(v) for v in x)
            min_dist = min(min_dist, d)
            if d <= max(DELTA_FLOOR, DELTA_FACTOR * e):
                firm = False
    pcm32 = np.ascontiguousarray(s.astype(np.int32).reshape(-1))
    nbits, best, w_best, comp = [], None, 0, None
    for w in range(5 if stereo else 1):
        d = desc(synth, n, cfg, ub=ub, coef_mode=1, mix_shift=2 if stereo else 0, mix_weight=w)
        d["coefs"][0, 0, :ORDER] = coefs[stream_a(stereo, w)]
        if stereo:
            d["coefs"][0, 1, :ORDER] = coefs[stream_b(w)]
        got = synth.encode_packet_bits(d, pcm32)
        nbits.append(None if got is None else got[1])
        if got is not None and (best is None or got[1] < best):
            best, w_best, comp = got[1], w, got[0]
    esc_pkt, esc_bits = synth.encode_packet_bits(desc(synth, n, cfg, escape=1), pcm32)
    margin = None if best is None else (esc_bits + 7) // 8 - (best + 7) // 8
    escape = margin is None or margin <= 0
    return Ref(packet=esc_pkt if escape else comp, samples=s, weight=w_best, escape=escape, coefs=coefs, nbits=nbits,
               comp_bits=best, esc_bits=esc_bits, margin=margin, firm=firm, min_dist=min_dist, err64=err64)

