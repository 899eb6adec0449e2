"""Smoothed fundamental frequency behind the crops: probabilistic YIN (Mauch and Dixon, ICASSP 2014 -- what `librosa.pyin`
computes), two launches (alacgpu_pyin_device, csrc/alac_pyin.hip): the observation of every frame, then a Viterbi decode along
every line.  librosa is not at hand where this is built: the parity is with this written specification, and the deviations
from `librosa.pyin` are listed at the end.

PYin(sample_rate, win_length, hop_length, fmin, fmax, n_thresholds = N, beta = (a, b), boltzmann = l, resolution,
max_transition_rate, switch_prob, no_trough_prob, center, align_length).  The framing, the lags tau_min .. tau_max, `span`,
`frames`, `lengths`, `min_frames` and `short` are those of the yin.Yin with the same first five arguments, center and
align_length (`PYin.yin`), and are taken from it.  Derived:

    nbps   = ceil(1 / resolution)                                   bins per semitone
    n_bins = floor(12 nbps log2(fmax / fmin)) + 1                   at most 1024
    h      = round(max_transition_rate * 12 * hop / sample_rate) * nbps      the half-width of the transition band
    f_b    = fmin * 2^(b / (12 nbps)),  b = 0 .. n_bins - 1         the bin frequencies
    K_max  = (tau_max - tau_min + 1) // 2                           the most troughs a frame can have (no two are neighbours)

The tables, each evaluated in float64 and rounded once to float32 (`PYin.tables`); the specification computes in float64 ON
THESE FLOAT32 VALUES, as `yin_host` does on the float32 threshold, so that it and the twin differ by the arithmetic alone:

    s_i      = i / N,  i = 1 .. N                                   the thresholds
    beta_i   = I(i / N) - I((i - 1) / N)                            I the CDF of Beta(a, b): for integers a, b the finite sum
                                                                    sum_{j = a}^{a+b-1} C(a+b-1, j) x^j (1 - x)^(a+b-1-j)
    cb_m     = beta_1 + .. + beta_m (of the float32 beta_i), m = 0 .. N
    bz_p     = (1 - e^-l) e^(-l p),  p = 0 .. K_max                 the Boltzmann factor of position p
    inv_n    = 1 / (1 - e^(-l n)),   n = 1 .. K_max (inv_0 = 0, never used)     its truncation to n positions
    edge_e   = sample_rate / (fmin 2^((e + 1/2) / (12 nbps))),  e = 0 .. n_bins - 2     period edges, descending
    lt_o     = log2((h + 1 - o) / (h + 1)),  o = 0 .. min(h, n_bins - 1)
    lz_j     = log2(Z_j),  Z_j = sum of (h + 1 - |i - j|) / (h + 1) over the bins i with |i - j| <= h that exist
    ls       = log2(1 - switch_prob), log2(switch_prob);   lstart = log2(1 / (2 n_bins))

Per frame, the observation:

    1.  d' [0 .. tau_max]: exactly steps 1 and 2 of yin.py (`yin._dprime_f64`, `yin._dprime_f32`)
    2.  troughs: every tau in tau_min .. tau_max - 1 with d'[tau] < d'[tau - 1] and d'[tau] <= d'[tau + 1], numbered k = 0, 1, ..
        by ascending lag.  The compares are IEEE's: a NaN is never a trough, nor is a neighbour of one.  A silent frame
        (c[tau_max] == 0, d' = 1 everywhere) has none.  Height h_k = d'[tau_k]; period = tau_k + shift_k with yin.py's step 4:
        a, b, c = d'[tau - 1], d'[tau], d'[tau + 1], shift = 0.5 (a - c) / (a - 2 b + c) when b <= a, b <= c and the denominator
        is positive, else 0
    3.  m_k = the number of i with not (h_k < s_i).  Trough k is below threshold i exactly when m_k < i; n_i = the number of
        troughs below i; pos_i(k) = the number of troughs k' < k below i
    4.  P_k = sum over i > m_k of beta_i * bz_{pos_i(k)} * inv_{n_i}.  The first trough of the least height gains
        no_trough_prob * cb_{m_k}: the weight of the thresholds no trough is below
    5.  the bin of trough k = the number of edges e with period_k < edge_e: a period exactly on an edge belongs to the lower bin
        (the lower frequency); below every edge it is n_bins - 1, at or above edge_0 it is 0.  p_b = the sum of the P_k of bin b,
        added in ascending k
    6.  vp = min(P_0 + P_1 + .., 1), added in ascending k from 0.  In the log2 domain: voiced state b observes
        log2(max(p_b, 2^-126)), every unvoiced state log2(max((1 - vp) / n_bins, 2^-126))

Across the frames of a line, the decode.  2 n_bins states: voiced 0 .. n_bins - 1, unvoiced n_bins .. 2 n_bins - 1, state s
has bin s mod n_bins.  Within a half T[j -> i] = tri(i - j) / Z_j, tri(o) = (h + 1 - |o|) / (h + 1) for |o| <= h and 0
otherwise: the rows are normalised at the edges, nothing wraps.  Between the halves 1 - switch_prob to stay and switch_prob to
switch (the Kronecker product of the two).  The start is uniform.  In log2, with obs_t[s] the observation of state s:

    delta_0[s] = lstart + obs_0[s]
    e[j]       = delta_{t-1}[j] - lz[j mod n_bins]                                  once per frame and state
    M_v(i)     = max over the voiced j with |i - j| <= h of e[j] + lt[|i - j|];    M_u(i) the same over the unvoiced j
    voiced i:    the larger of M_v(i) + ls[0] and M_u(i) + ls[1];   unvoiced i: of M_v(i) + ls[1] and M_u(i) + ls[0]
    delta_t[s] = obs_t[s] + that

and the source state is remembered.  Every tie goes to the lowest source state in the order 0 .. 2 n_bins - 1: within a band
the lowest j, between the halves the voiced one, in the final arg-max over delta_{T'-1} the first -- `np.argmax`'s rule, which
the twin and the kernel both follow: a candidate replaces the best so far only when it is strictly larger, and candidates come
in ascending order.  The path is walked back from that arg-max.

The output is float32 [B, C, 3, T'] (T' = frames(T)): line 0 the decoded state's bin frequency f_b in Hz -- always a number,
as `Yin`'s line 0 is --, line 1 1.0 where the state is voiced and 0.0 where not (`PYin.voiced`), line 2 vp.  Frames at and
behind the line's frame count are zeros in all three; a line with no frames is zeros and runs no recursion.

`pyin_host` is the above in float64 on the float32 input.  `pyin_host_f32` is the kernels, operation by operation, and equals
them bit for bit (fl: one float32 rounding; nothing is contracted, the divisions are correctly rounded):

    2.  n = fl(a - c), q = fl(fl(a - 2 b) + c), shift = fl(fl(0.5 n) / q), period = fl(float(tau) + shift): yin.py's
    4.  threshold i belongs to lane (i - 1) mod 64.  A lane adds its terms fl(fl(beta_i bz_pos) inv_n), i ascending, from 0:
        part = fl(part + term); the 64 parts are then added as a tree of halves, part[l] = fl(part[l] + part[l + w]) for
        w = 32, 16, 8, 4, 2, 1, and P_k is part[0].  (A threshold at or under m_k adds nothing.)  The gain of the least trough:
        P_k = fl(P_k + fl(no_trough_prob cb_m)), cb from the table
    5.  p_b = fl(p_b + P_k), k ascending
    6.  vp: v = fl(v + P_k) from 0, k ascending, then min(v, 1);  unvoiced: fl(fl(1 - vp) / float(n_bins));  log2 is the
        explicit polynomial of pcen.py (`pcen._log2_f32`, alac_pcen_log2), applied to max(p, 2^-126): an empty bin is exactly -126
    decode: every sum and difference above is one fl(), in the order written: e = fl(delta - lz), fl(e + lt), fl(M + ls),
        fl(obs + .), delta_0 = fl(lstart + obs_0)

`specification` and `twin` here mean those two.  The float64 specification uses the same order of sums; at 2^-53 the order is
not visible in anything below.

The bounds, with u = 2^-24 and gamma_k = k u / (1 - k u).  d' is within E = `yin.dprime_bound` of the specification's,
relatively, in any correct float32 evaluation.  The data-dependent choices of a frame's observation are compares of two such
values: the two trough compares of EVERY candidate lag (not only of the troughs: a flip makes or removes one), the compare of
each trough's height with each threshold s_i (exact), and of the least height with the other troughs' heights (who gains
no_trough_prob).  The margin of a frame (`pyin_host(..., details=True)["margin"]`) is the smallest |p - q| / (|p| + |q|) over
all of them (|h - s_i| / |h| for a threshold), yin.py's notion extended; a frame whose margin exceeds E has the same troughs,
the same m_k, n_i and pos_i(k) and the same least trough in any correct float32 evaluation (step 4's own compares b <= a,
b <= c hold for a trough by definition, and then q = (a - b) + (c - b) > 0).  Then P_k is a sum of non-negative terms, each
a product of table values with two roundings, added through at most ceil(N / 64) + 6 sums, and the gain costs a product and a
sum more:

    |P_k' - P_k| <= gamma_{ceil(N / 64) + 10} P_k + (3 N + 8) 2^-150                                   (`pk_bound`, `pk_floor`)

The second term is the underflow's: a product or sum that lands under 2^-126 is rounded to a multiple of 2^-149, at most 2^-150
off whatever its size, and a P_k passes at most 2 N products, N sums and the 8 operations of the tree and the gain.  It matters
only to troughs whose probability is itself of that order (the Boltzmann factor of position 40 at l = 2 is e^-80).

The decode.  With A = 126 + max |lz| + max |lt| + max |ls| a step moves delta by at most A, so every value the recursion
rounds is at most V = |lstart| + 126 + (T' - 1) A in magnitude (the tables' values are float32 already and add no error).  A
path's float32 score passes four roundings per frame (e, + lt, + ls, + obs), each at most u V: its computed score is within
R = 4 T' u V (1 + 2^-20) of its float64 score ON THE SAME OBSERVATIONS.  The path the float32 recursion keeps has a computed
score at least that of the optimum's path, so its float64 score falls short of the float64 optimum by at most

    D(T') = 2 R = 8 T' u V (1 + 2^-20)                                                                  (`decode_bound`)

(both scores on the twin's observations: the bound is about the recursion; how far the observations are from the
specification's is `pk_bound` and the polynomial's 4 u of pcen.py.)

What differs from `librosa.pyin`: the framing is `Yin`'s (zeros outside the crop, span = W + tau_max, no reflection); the
trough rule compares with the real neighbour d'[tau_min - 1] at tau_min where librosa takes y[0] < y[1]; h is the half-width of
the band; a trough's bin is clipped to n_bins - 1, not n_bins; colliding troughs add where librosa overwrites; the floor of a
probability is 2^-126, not float64's tiny; the Beta parameters are integers; there is no `fill_na`: line 0 is always a number.

The backpointers of the decode are uint16 [B C, T', 2 n_bins] beside the observations in the context's scratch: ValueError
where that scratch would pass 2^31 bytes.

`PYin`, `pyin_host`, `pyin_host_f32`, `pyin_decode_host`, `path_score`, `pk_bound`, `pk_floor` and `decode_bound` need no device; `pyin`,
`pyin_observation` and `pyin_decode` are the calls on device tensors.
"""
import math

import numpy as np

from ._stageargs import _device_context, _f32_finite, _lengths_device, _lengths_host, _planes, _span, _Spec
from .pcen import _log2_f32
from .yin import Yin, _dprime_f32, _dprime_f64, _gamma, _int, _rel, _segments, dprime_bound, tile_frames

_U = 2.0 ** -24
MAX_BINS, MAX_THRESHOLDS = 1024, 256               # ALAC_PYIN_MAX_BINS, ALAC_PYIN_MAX_THRESHOLDS of csrc/alac_pyin.h
FLOOR = 2.0 ** -126
SCRATCH_MAX = 1 << 31
_TABLE_ORDER = ("s", "beta", "cb", "bz", "inv", "edges", "freq", "lz", "lt", "ls", "lstart")    # alac_pyin_tables of csrc/alac_pyin.h
_TABLES = {}                                       # (spec, device index) -> the packed float32 device tensor


class PYin(_Spec):
    """An immutable description of the pYIN estimator (see the module).  ValueError: whatever `Yin` refuses for the framing
    and the lags, n_thresholds outside 1 .. 256, beta no pair of positive integers with a + b <= 64, boltzmann not above 0,
    resolution outside (0, 1], max_transition_rate below 0, switch_prob outside (0, 1), no_trough_prob outside [0, 1],
    more than 1024 bins, a number that is not finite in float32."""

    __slots__ = ("yin", "n_thresholds", "beta", "boltzmann", "resolution", "max_transition_rate", "switch_prob", "no_trough_prob")

    def __init__(self, sample_rate, win_length=512, hop_length=160, fmin=60.0, fmax=400.0, n_thresholds=100, beta=(2, 18), boltzmann=2.0,
                 resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, center=True, align_length=None):
        s = object.__setattr__
        s(self, "yin", Yin(sample_rate, win_length, hop_length, fmin, fmax, center=center, align_length=align_length))
        s(self, "n_thresholds", _int("n_thresholds", n_thresholds, 1, MAX_THRESHOLDS))
        if not isinstance(beta, (tuple, list)) or len(beta) != 2:
            raise ValueError(f"beta must be two positive integers with a + b <= 64, not {beta!r}")
        a, b = (_int("beta", v, 1) for v in beta)
        if a + b > 64:
            raise ValueError(f"beta must be two positive integers with a + b <= 64, not {beta!r}")
        s(self, "beta", (a, b))
        l = _f32_finite("boltzmann", boltzmann)
        if not l > 0.0:
            raise ValueError(f"boltzmann must be above 0, not {boltzmann!r}")
        s(self, "boltzmann", l)
        r = _f32_finite("resolution", resolution)
        if not 0.0 < r <= 1.0:
            raise ValueError(f"resolution must be in (0, 1], not {resolution!r}")
        s(self, "resolution", r)
        s(self, "max_transition_rate", _f32_finite("max_transition_rate", max_transition_rate, 0.0))
        sp = _f32_finite("switch_prob", switch_prob)
        if not 0.0 < sp < 1.0 or not 0.0 < float(np.float32(sp)) < 1.0:
            raise ValueError(f"switch_prob must be in (0, 1), not {switch_prob!r}")
        s(self, "switch_prob", sp)
        nt = _f32_finite("no_trough_prob", no_trough_prob)
        if not 0.0 <= nt <= 1.0:
            raise ValueError(f"no_trough_prob must be in [0, 1], not {no_trough_prob!r}")
        s(self, "no_trough_prob", nt)
        if self.n_bins > MAX_BINS:
            raise ValueError(f"fmin {fmin!r}, fmax {fmax!r} at resolution {resolution!r}: {self.n_bins} bins are above {MAX_BINS}")

    @classmethod
    def like(cls, spec, **kw):
        """The PYin whose frames are those of `spec`: what `Yin.like` takes and refuses.  kw: the other arguments of `PYin`."""
        return Yin.like.__func__(cls, spec, **kw)

    # the framing and the lags: the Yin's
    sample_rate = property(lambda self: self.yin.sample_rate)
    win_length = property(lambda self: self.yin.win_length)
    hop_length = property(lambda self: self.yin.hop_length)
    fmin = property(lambda self: self.yin.fmin)
    fmax = property(lambda self: self.yin.fmax)
    center = property(lambda self: self.yin.center)
    align_length = property(lambda self: self.yin.align_length)
    tau_min = property(lambda self: self.yin.tau_min)
    tau_max = property(lambda self: self.yin.tau_max)
    span = property(lambda self: self.yin.span)
    first = property(lambda self: self.yin.first)
    min_frames = property(lambda self: self.yin.min_frames)

    def frames(self, L):
        return self.yin.frames(L)

    def short(self, L):
        return self.yin.short(L)

    def lengths(self, lengths):
        return self.yin.lengths(lengths)

    @property
    def nbps(self):
        """Bins per semitone: ceil(1 / resolution)"""
        return math.ceil(1.0 / self.resolution)

    @property
    def n_bins(self):
        return math.floor(12 * self.nbps * math.log2(self.fmax / self.fmin)) + 1

    @property
    def h(self):
        """The half-width of the transition band in bins"""
        return round(self.max_transition_rate * 12 * self.hop_length / self.sample_rate) * self.nbps

    @property
    def band(self):
        """min(h, n_bins - 1): the offsets that exist"""
        return min(self.h, self.n_bins - 1)

    @property
    def max_troughs(self):
        return (self.tau_max - self.tau_min + 1) // 2

    def weights(self):
        """beta_i, i = 1 .. N, in float64: the Beta(a, b) CDF's differences over the thresholds"""
        a, b = self.beta
        m, N = a + b - 1, self.n_thresholds
        term = lambda x, j: math.comb(m, j) * x ** j * (1.0 - x) ** (m - j)
        # the CDF from below and its complement from above, each a sum of positive terms; a weight is the difference of
        # whichever pair is the smaller, so none loses its digits against 1
        low = [0.0] + [math.fsum(term(i / N, j) for j in range(a, m + 1)) for i in range(1, N)] + [1.0]
        high = [1.0] + [math.fsum(term(i / N, j) for j in range(a)) for i in range(1, N)] + [0.0]
        return np.asarray([low[i] - low[i - 1] if low[i] < 0.5 else high[i - 1] - high[i] for i in range(1, N + 1)])

    def boltzmann_factors(self, n):
        """The truncated Boltzmann distribution over n positions in float64: bz_p inv_n, p = 0 .. n - 1"""
        l = self.boltzmann
        return -math.expm1(-l) * np.exp(-l * np.arange(n)) / -math.expm1(-l * n)

    def transition(self):
        """T[j, i] within a half, float64 [n_bins, n_bins]: tri(i - j) / Z_j"""
        n, h = self.n_bins, self.h
        o = np.abs(np.arange(n)[None, :] - np.arange(n)[:, None])
        tri = np.where(o <= h, (h + 1.0 - o) / (h + 1.0), 0.0)
        return tri / tri.sum(axis=1, keepdims=True)

    def tables(self):
        """The float32 tables of the module by name, each from float64 and rounded once"""
        f32 = np.float32
        N, n, K, l, h = self.n_thresholds, self.n_bins, self.max_troughs, self.boltzmann, self.h
        beta = self.weights().astype(f32)
        step = 12.0 * self.nbps
        o = np.abs(np.arange(n)[None, :] - np.arange(n)[:, None])
        Z = np.where(o <= h, (h + 1.0 - o) / (h + 1.0), 0.0).sum(axis=1)
        with np.errstate(all="ignore"):
            inv = np.concatenate([[0.0], 1.0 / -np.expm1(-l * np.arange(1, K + 1))])
        sp = float(f32(self.switch_prob))
        t = dict(s=np.arange(1, N + 1) / N, beta=beta, cb=np.concatenate([[0.0], np.cumsum(beta.astype(np.float64))]),
                 bz=-math.expm1(-l) * np.exp(-l * np.arange(K + 1)), inv=inv,
                 edges=self.sample_rate / (self.fmin * 2.0 ** ((np.arange(n - 1) + 0.5) / step)),
                 freq=self.fmin * 2.0 ** (np.arange(n) / step), lz=np.log2(Z),
                 lt=np.log2((h + 1.0 - np.arange(self.band + 1)) / (h + 1.0)), ls=np.log2(np.asarray([1.0 - sp, sp])),
                 lstart=np.asarray([math.log2(1.0 / (2 * n))]))
        return {k: np.ascontiguousarray(t[k], dtype=f32) for k in _TABLE_ORDER}

    def table(self):
        """The tables packed in the order of alac_pyin_tables (csrc/alac_pyin.h): alacgpu_pyin_device's d_table"""
        t = self.tables()
        return np.concatenate([t[k] for k in _TABLE_ORDER])

    def voiced(self, y):
        """Which frames of y [..., 3, T'] (what `pyin` and the host functions return) are voiced: line 1, as a boolean [..., T']"""
        return y[..., 1, :] != 0


def pk_bound(spec):
    """How far a P_k of any correct float32 evaluation is from the specification's, relatively, on a frame whose margin exceeds
    `yin.dprime_bound(spec.yin)` (the module docstring)"""
    return _gamma((spec.n_thresholds + 63) // 64 + 10)


def pk_floor(spec):
    """The absolute term beside `pk_bound`: what the roundings of subnormal products and sums add to a P_k at most"""
    return (3 * spec.n_thresholds + 8) * 2.0 ** -150


def decode_bound(spec, frames):
    """D(T') of the module: how much the float64 score of the float32 recursion's path may fall short of the float64 optimum
    on the same observations, for a line of `frames` frames"""
    t = {k: v.astype(np.float64) for k, v in spec.tables().items()}
    A = 126.0 + np.max(np.abs(t["lz"])) + np.max(np.abs(t["lt"])) + np.max(np.abs(t["ls"]))
    V = abs(float(t["lstart"][0])) + 126.0 + max(frames - 1, 0) * A
    return 8.0 * frames * _U * V * (1.0 + 2.0 ** -20)


# ---- the observation of a frame ------------------------------------------------------------------------------------------------
def _lane_tree(term, f):
    """term [K, N] added over the thresholds in the module's order: threshold i in lane (i - 1) % 64, a lane's terms ascending,
    then the tree of halves over the lanes"""
    K, N = term.shape
    J = (N + 63) // 64
    pad = np.zeros((K, J * 64), dtype=f)
    pad[:, :N] = term
    pad = pad.reshape(K, J, 64)
    part = np.zeros((K, 64), dtype=f)
    for j in range(J):
        part = (part + pad[:, j]).astype(f)
    w = 32
    while w >= 1:
        part = (part[:, :w] + part[:, w:2 * w]).astype(f)
        w //= 2
    return part[:, 0]


def _observe(dp, spec, T, f, margin):
    """Steps 2 to 6 of a frame on d' [tau_max + 1] in the arithmetic `f` with the tables T (values of dtype f): the troughs'
    lags, P_k and bins, p [n_bins], vp, and the frame's margin (inf without `margin`)"""
    lo, hi, n = spec.tau_min, spec.tau_max - 1, spec.n_bins
    with np.errstate(all="ignore"):
        a, b, c = dp[lo - 1:hi], dp[lo:hi + 1], dp[lo + 1:hi + 2]
        taus = lo + np.nonzero((b < a) & (b <= c))[0]
        m_all = np.inf
        if margin:
            m_all = float(min(np.min(_rel(b.astype(np.float64), a.astype(np.float64))), np.min(_rel(b.astype(np.float64), c.astype(np.float64)))))
        K = len(taus)
        p = np.zeros(n, dtype=f)
        if K == 0:
            return taus, np.zeros(0, dtype=f), np.zeros(0, dtype=np.int64), p, f(0.0), m_all
        h = dp[taus]
        below = ~(h[:, None] < T["s"][None, :])                       # [K, N]: not (h_k < s_i)
        m = below.sum(axis=1)
        below = m[:, None] < np.arange(1, spec.n_thresholds + 1)[None, :]
        pos = np.cumsum(below, axis=0) - below
        cnt = below.sum(axis=0)
        term = ((T["beta"][None, :] * T["bz"][pos]).astype(f) * T["inv"][cnt][None, :]).astype(f)
        P = _lane_tree(np.where(below, term, f(0.0)).astype(f), f)
        k0 = int(np.argmin(h))
        cb = T["cb"][m[k0]] if f is np.float32 else np.sum(T["beta"][:m[k0]])
        P[k0] = f(P[k0] + f(f(np.float32(spec.no_trough_prob)) * cb))
        if margin:
            hh = h.astype(np.float64)
            r = np.abs(hh[:, None] - T["s"][None, :]) / np.abs(hh[:, None])
            m_all = min(m_all, float(np.min(np.where(np.isnan(r), np.inf, r))))
            if K > 1:
                m_all = min(m_all, float(np.min(_rel(np.delete(hh, k0), hh[k0]))))
        aa, cc = dp[taus - 1], dp[taus + 1]
        nn = (aa - cc).astype(f)
        q = ((aa - (f(2.0) * h).astype(f)).astype(f) + cc).astype(f)
        ok = (h <= aa) & (h <= cc) & (q > 0)
        shift = np.where(ok, ((f(0.5) * nn).astype(f) / np.where(ok, q, f(1.0))).astype(f), f(0.0)).astype(f)
        period = (taus.astype(f) + shift).astype(f)
        bins = (period[:, None] < T["edges"][None, :]).sum(axis=1)
        v = f(0.0)
        for k in range(K):
            p[bins[k]] = f(p[bins[k]] + P[k])
            v = f(v + P[k])
    return taus, P, bins, p, min(v, f(1.0)), m_all


def _to_log2(p, vp, n, f):
    """Step 6: the voiced observations of p [.., n_bins] and the unvoiced one of vp [..]"""
    with np.errstate(all="ignore"):
        u = ((f(1.0) - vp).astype(f) / f(n)).astype(f)
        if f is np.float32:
            return _log2_f32(np.maximum(p, f(FLOOR))), _log2_f32(np.maximum(u, f(FLOOR)))
        return np.log2(np.maximum(p, FLOOR)), np.log2(np.maximum(u, FLOOR))


def _host_args(x, spec, lengths):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim not in (2, 3):
        raise ValueError(f"x must be float32 [B, C, T] or [B, T], not {x.dtype} {x.shape}")
    if not isinstance(spec, PYin):
        raise ValueError(f"spec must be a PYin, not {spec!r}")
    x3 = x if x.ndim == 3 else x[:, None, :]
    return x3, x.ndim == 3, _lengths_host("lengths", lengths, x.shape[0], x.shape[-1])


# ---- the decode ----------------------------------------------------------------------------------------------------------------
def _decode(ov, ou, counts, spec, f):
    """The recursion and the walk back on ov [P, T', n_bins], ou [P, T'] (log2 observations of dtype f) for lines of counts [P]
    frames: int32 states [P, T'], -1 at and behind a line's count.  Every tie to the lowest source state."""
    T = {k: v.astype(f) for k, v in spec.tables().items()}
    n, band = spec.n_bins, spec.band
    Pn, Tn = ou.shape
    states = np.full((Pn, Tn), -1, dtype=np.int32)
    most = int(counts.max()) if Pn else 0
    if most == 0:
        return states
    obs = np.concatenate([ov, np.broadcast_to(ou[:, :, None], ov.shape)], axis=2).astype(f)
    bp = np.zeros((Pn, most, 2 * n), dtype=np.int32)
    last = np.zeros(Pn, dtype=np.int64)
    lz, lt, ls = T["lz"], T["lt"], T["ls"]
    at = np.arange(n)
    with np.errstate(all="ignore"):
        delta = (T["lstart"][0] + obs[:, 0]).astype(f)
        for t in range(most):
            if t:
                e = (delta.reshape(Pn, 2, n) - lz[None, None, :]).astype(f)
                M = np.full((Pn, 2, n), -np.inf, dtype=f)
                arg = np.zeros((Pn, 2, n), dtype=np.int32)
                for o in range(-band, band + 1):                            # the source j = i + o, ascending
                    i0, i1 = max(0, -o), min(n, n - o)
                    cand = (e[:, :, i0 + o:i1 + o] + lt[abs(o)]).astype(f)
                    better = cand > M[:, :, i0:i1]
                    M[:, :, i0:i1] = np.where(better, cand, M[:, :, i0:i1])
                    arg[:, :, i0:i1] = np.where(better, (at[i0:i1] + o)[None, None, :], arg[:, :, i0:i1])
                best, src = [], []
                for half in (0, 1):                                         # the targets of the voiced half, then of the unvoiced
                    a = (M[:, 0] + ls[half]).astype(f)
                    b = (M[:, 1] + ls[1 - half]).astype(f)
                    take = b > a                                            # a tie: the voiced source
                    best.append(np.where(take, b, a))
                    src.append(np.where(take, n + arg[:, 1], arg[:, 0]))
                delta = (obs[:, t] + np.concatenate(best, axis=1)).astype(f)
                bp[:, t] = np.concatenate(src, axis=1)
            ends = counts == t + 1
            if ends.any():
                last[ends] = np.argmax(delta[ends], axis=1)
    for r in range(Pn):
        s = int(last[r])
        for t in range(int(counts[r]) - 1, -1, -1):
            states[r, t] = s
            s = int(bp[r, t, s])
    return states


def _decode_args(obs_voiced, obs_unvoiced, spec, frame_counts):
    ov, ou = np.asarray(obs_voiced), np.asarray(obs_unvoiced)
    if not isinstance(spec, PYin):
        raise ValueError(f"spec must be a PYin, not {spec!r}")
    if ov.ndim != 4 or ov.shape[3] != spec.n_bins or ou.shape != ov.shape[:3]:
        raise ValueError(f"obs_voiced must be [B, C, T', {spec.n_bins}] and obs_unvoiced [B, C, T'], not {ov.shape} and {ou.shape}")
    B, C, Tn, n = ov.shape
    counts = np.repeat(_lengths_host("frame_counts", frame_counts, B, Tn), C)
    return ov.reshape(B * C, Tn, n), ou.reshape(B * C, Tn), counts, (B, C, Tn)


def pyin_decode_host(obs_voiced, obs_unvoiced, spec, frame_counts=None, f32=False):
    """The decode alone in numpy: obs_voiced [B, C, T', n_bins] and obs_unvoiced [B, C, T'], log2 observations, to the int32
    states [B, C, T'] of the best path, -1 at and behind a row's frame_counts [B] (default: T').  f32: the kernel's float32
    recursion, bit for bit (the observations as float32); else float64."""
    f = np.float32 if f32 else np.float64
    ov, ou, counts, shape = _decode_args(obs_voiced, obs_unvoiced, spec, frame_counts)
    return _decode(ov.astype(f), ou.astype(f), counts, spec, f).reshape(shape)


def path_score(obs_voiced, obs_unvoiced, states, spec, frame_counts=None):
    """The float64 log2 score of the paths `states` [B, C, T'] on those observations [B, C] (the tables' float32 values, float64
    sums): lstart + obs_0 + the transitions and observations behind; -inf for a step outside the band, 0 for a line without
    frames"""
    ov, ou, counts, shape = _decode_args(obs_voiced, obs_unvoiced, spec, frame_counts)
    T = {k: v.astype(np.float64) for k, v in spec.tables().items()}
    n, band = spec.n_bins, spec.band
    st = np.asarray(states).reshape(shape[0] * shape[1], shape[2])
    out = np.zeros(len(st))
    for r in range(len(st)):
        prev = None
        for t in range(int(counts[r])):
            s = int(st[r, t])
            o = float(ov[r, t, s]) if s < n else float(ou[r, t])
            if prev is None:
                out[r] += T["lstart"][0] + o
            else:
                d = abs(s % n - prev % n)
                step = T["lt"][d] - T["lz"][prev % n] if d <= band else -np.inf
                out[r] += step + T["ls"][0 if (s < n) == (prev < n) else 1] + o
            prev = s
    return out.reshape(shape[:2])


# ---- the two host functions ----------------------------------------------------------------------------------------------------
def _host(x, spec, lengths, f, details):
    x3, had_c, lens = _host_args(x, spec, lengths)
    B, C, Tx = x3.shape
    n, nf = spec.n_bins, int(spec.frames(Tx))
    T = {k: v.astype(f) for k, v in spec.tables().items()}
    P = np.zeros((B * C, nf, n), dtype=f)
    vp = np.zeros((B * C, nf), dtype=f)
    margins = np.full((B * C, nf), np.inf)
    troughs = [[None] * nf for _ in range(B * C)]
    counts = np.zeros(B * C, dtype=np.int64)
    tile = tile_frames(spec.yin)
    for b in range(B):
        v = int(lens[b])
        count = min(int(spec.frames(v)), nf)
        for ch in range(C):
            r = b * C + ch
            counts[r] = count
            for t0 in range(0, count, tile):
                t1 = min(t0 + tile, count)
                dp, _ = (_dprime_f32 if f is np.float32 else _dprime_f64)(_segments(x3[b, ch], v, spec.yin, t0, t1, f), spec.yin)
                for t in range(t0, t1):
                    taus, Pk, bins, P[r, t], vp[r, t], margins[r, t] = _observe(dp[t - t0], spec, T, f, details and f is np.float64)
                    troughs[r][t] = (taus, Pk, bins)
    ov, ou = _to_log2(P, vp, n, f)
    on = np.arange(nf)[None, :] < counts[:, None]
    ov, ou = np.where(on[:, :, None], ov, f(0.0)).astype(f), np.where(on, ou, f(0.0)).astype(f)
    states = _decode(ov, ou, counts, spec, f)
    y = np.zeros((B * C, 3, nf), dtype=f)
    y[:, 0] = np.where(on, T["freq"][np.maximum(states, 0) % n], f(0.0))
    y[:, 1] = np.where(on & (states < n), f(1.0), f(0.0))
    y[:, 2] = vp
    shape = (B, C) if had_c else (B,)
    y = y.reshape(shape + (3, nf))
    if not details:
        return y
    info = dict(states=states.reshape(shape + (nf,)), obs_voiced=ov.reshape(shape + (nf, n)), obs_unvoiced=ou.reshape(shape + (nf,)),
                vp=vp.reshape(shape + (nf,)), margin=margins.reshape(shape + (nf,)), troughs=troughs, frame_counts=counts.reshape(B, C)[:, 0])
    return y, info


def pyin_host(x, spec, lengths=None, details=False):
    """The specification in numpy: float64 [B, C, 3, T'] ([B, 3, T'] for x [B, T]) from x float32, float64 arithmetic on the
    float32 input and the float32 tables.  lengths: [B] integers (below 0 counts as 0, above T as T); default: T.
    details=True: returns (y, info), info a dict of `states` int32 [B, C, T'] (-1 behind a row's frames), `obs_voiced`
    [B, C, T', n_bins], `obs_unvoiced` and `vp` [B, C, T'] (zeros behind a row's frames), `margin` float64 [B, C, T'] as the
    module defines it, `frame_counts` [B], and `troughs`: per plane (row-major) and frame the tuple (lags, P_k, bins)."""
    return _host(x, spec, lengths, np.float64, details)


def pyin_host_f32(x, spec, lengths=None, details=False):
    """The kernels' arithmetic in numpy, bit for bit: float32 [B, C, 3, T'] ([B, 3, T'] for x [B, T]); details as for
    `pyin_host` (the margin is infinite: it belongs to the specification)"""
    return _host(x, spec, lengths, np.float32, details)


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _table_device(spec, device):
    """The packed float32 tables of a spec on a device: uploaded once per (spec, device) and kept, as pcen.py's"""
    import torch

    key = (spec, device.index if device.index is not None else torch.cuda.current_device())
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) >= 64:
            _TABLES.pop(next(iter(_TABLES)))
        t = _TABLES[key] = torch.from_numpy(spec.table()).to(device)
    return t


def _scratch_bytes(planes, frames, n_bins):
    """What stage 0 keeps in the context's scratch: the observations and the uint16 backpointers"""
    return 4 * planes * frames * (n_bins + 2) + 2 * planes * frames * 2 * n_bins


def _launch(ctx, spec, stage, stream, B, C, frames, n, **kw):
    a = dict(d_src=None, stride=0, d_valid=None, d_obs_voiced=None, d_obs_unvoiced=None, d_vp=None, d_out=None, d_states=None)
    a.update(kw)
    ctx().pyin_device(a["d_src"], B, C, a["stride"], frames, a["d_valid"], spec.sample_rate, spec.win_length, spec.hop_length, spec.tau_min,
                      spec.tau_max, 0 if spec.center else spec.align_length, spec.n_thresholds, spec.n_bins, spec.band,
                      spec.no_trough_prob, a["d_table"], a["d_obs_voiced"], a["d_obs_unvoiced"], a["d_vp"], a["d_out"], a["d_states"], n,
                      stage=stage, stream=stream)


def _checked(pcm, spec, lengths):
    import torch

    if not isinstance(spec, PYin):
        raise ValueError(f"spec must be a PYin, not {spec!r}")
    stride = _planes("pcm", pcm)
    B, C, T = pcm.shape
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    return stride, B, C, T, int(spec.frames(T)), _lengths_device("lengths", lengths, B, pcm.device)


def _pyin(ctx, pcm, spec, lengths, out):
    """`pyin` behind its first check, on pcm [B, C, T]; ctx() gives the context that runs it (the corpus's own inside
    `Corpus.crops`); out: a contiguous float32 tensor [B, C, 3, T'] to write, or None for a new one"""
    import torch

    stride, B, C, T, n, d_valid = _checked(pcm, spec, lengths)
    shape = (B, C, 3, n)
    if _scratch_bytes(B * C, n, spec.n_bins) > SCRATCH_MAX:
        raise ValueError(f"{B * C} lines of {n} frames and {spec.n_bins} bins: the observations and backpointers would pass 2^31 bytes")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    else:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != pcm.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {pcm.device}")
        if pcm.numel() and out.numel():
            (x0, x1), o0 = _span(pcm, stride), out.data_ptr()
            if x0 < o0 + 4 * out.numel() and o0 < x1:
                raise ValueError("out overlaps pcm")
    if out.numel() == 0:
        return out
    if T == 0:                       # (centred: one frame a row, of silence: the first unvoiced state; the library takes no empty planes)
        out[:, :, 0, :] = float(spec.tables()["freq"][0])
        out[:, :, 1:, :] = 0.0
        return out
    with torch.cuda.device(pcm.device):
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _launch(ctx, spec, 0, stream, B, C, T, n, d_src=pcm, stride=stride, d_valid=d_valid, d_table=_table_device(spec, pcm.device), d_out=out)
    return out


def pyin(pcm, spec, lengths=None, out=None):
    """The smoothed F0 track on the GPU: pcm float32 [B, C, T] or [B, T] on the device, contiguous or the slice [..., :T] of a
    contiguous tensor (what lies behind the slice is not read); spec: a `PYin`; lengths: [B] integers, a sequence or a tensor
    (-1 counts as 0, more than T as T); default: T.  Returns float32 [B, C, 3, T'] ([B, 3, T'] for [B, T]), T' =
    spec.frames(T): the decoded bin's frequency in Hz, 1.0 where voiced, the voicing probability; zeros at and behind the
    row's frame count (see the module).  out: a contiguous tensor of that shape apart from pcm; default: a new one.  Two
    launches, asynchronous on the current stream, nothing is read back; the observations and the uint16 backpointers
    [B C, T', 2 n_bins] live in the context's scratch: ValueError where they would pass 2^31 bytes, and for every other bad
    argument, before any device work."""
    import torch

    ctx = _device_context("pcm", pcm, "[B, C, T] or [B, T]")
    if pcm.dim() == 2:
        if out is not None and (not isinstance(out, torch.Tensor) or out.dim() != 3):
            raise ValueError("out must be a contiguous float32 tensor [B, 3, T']")
        return _pyin(ctx, pcm[:, None, :], spec, lengths, None if out is None else out[:, None])[:, 0]
    return _pyin(ctx, pcm, spec, lengths, out)


def pyin_observation(pcm, spec, lengths=None):
    """The first launch alone: pcm and lengths as for `pyin` to (obs_voiced float32 [B, C, T', n_bins], obs_unvoiced
    [B, C, T'], vp [B, C, T']) -- the log2 observations of the voiced states and of every unvoiced state, and the voicing
    probability; zeros at and behind a row's frame count.  [B, T] counts as [B, 1, T]."""
    import torch

    ctx = _device_context("pcm", pcm, "[B, C, T] or [B, T]")
    if pcm.dim() == 2:
        pcm = pcm[:, None, :]
    stride, B, C, T, n, d_valid = _checked(pcm, spec, lengths)
    ov = torch.zeros((B, C, n, spec.n_bins), dtype=torch.float32, device=pcm.device)
    ou = torch.zeros((B, C, n), dtype=torch.float32, device=pcm.device)
    vp = torch.zeros((B, C, n), dtype=torch.float32, device=pcm.device)
    if ou.numel() == 0:
        return ov, ou, vp
    if T == 0:                       # (centred: one frame of silence)
        ov[:] = -126.0
        ou[:] = float(_log2_f32(np.float32(1.0) / np.float32(spec.n_bins)))
        return ov, ou, vp
    with torch.cuda.device(pcm.device):
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _launch(ctx, spec, 1, stream, B, C, T, n, d_src=pcm, stride=stride, d_valid=d_valid, d_table=_table_device(spec, pcm.device),
                d_obs_voiced=ov, d_obs_unvoiced=ou, d_vp=vp)
    return ov, ou, vp


def pyin_decode(obs_voiced, obs_unvoiced, spec, frame_counts=None):
    """The second launch alone, on given observations: obs_voiced float32 [B, C, T', n_bins] and obs_unvoiced [B, C, T'],
    contiguous device tensors of finite log2 observations; frame_counts: [B] integers, a sequence or a tensor (below 0 counts
    as 0, more than T' as T'); default: T'.  Returns the int32 states [B, C, T'] of the best path, -1 at and behind a row's
    count (`pyin_decode_host` with f32=True, bit for bit).  ValueError where the backpointers would pass 2^31 bytes."""
    import torch

    ctx = _device_context("obs_voiced", obs_voiced, "[B, C, T', n_bins]")
    if not isinstance(spec, PYin):
        raise ValueError(f"spec must be a PYin, not {spec!r}")
    ov, ou = obs_voiced, obs_unvoiced
    if (ov.dtype != torch.float32 or ov.dim() != 4 or ov.shape[3] != spec.n_bins or ov.shape[1] == 0 or not ov.is_contiguous()
            or not isinstance(ou, torch.Tensor) or ou.dtype != torch.float32 or ou.device != ov.device or tuple(ou.shape) != tuple(ov.shape[:3])
            or not ou.is_contiguous()):
        raise ValueError(f"obs_voiced must be a contiguous float32 device tensor [B, C, T', {spec.n_bins}] and obs_unvoiced [B, C, T'] beside it")
    B, C, n, _ = ov.shape
    if frame_counts is not None and not isinstance(frame_counts, torch.Tensor):
        _lengths_host("frame_counts", frame_counts, B, n)
    d_counts = _lengths_device("frame_counts", frame_counts, B, ov.device)
    if 2 * B * C * n * 2 * spec.n_bins > SCRATCH_MAX:
        raise ValueError(f"{B * C} lines of {n} frames and {spec.n_bins} bins: the backpointers would pass 2^31 bytes")
    states = torch.full((B, C, n), -1, dtype=torch.int32, device=ov.device)
    if states.numel() == 0:
        return states
    with torch.cuda.device(ov.device):
        stream = torch.cuda.current_stream(ov.device).cuda_stream
        _launch(ctx, spec, 2, stream, B, C, n, n, d_valid=d_counts, d_table=_table_device(spec, ov.device), d_obs_voiced=ov, d_obs_unvoiced=ou,
                d_states=states)
    return states
