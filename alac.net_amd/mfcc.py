"""Kaldi MFCC features behind the decode: the fbank kernel's framing, mean, pre-emphasis, window, DFT and mel projection, and
in the same launch the log, the DCT, the lifter and the frame's energy (alacgpu_mfcc_device, csrc/alac_mfcc.hip).  What
Kaldi's `compute-mfcc-feats`, torchaudio.compliance.kaldi.mfcc, lhotse's `Mfcc` and the x-vector, diarisation, language-ID and
hybrid recipes built on them compute.

Frames, s, mu, d, y, a, X, P and M are fbank.py's, which states them, their tables and their float32 order; `use_power` picks
P or its root as there, and the log is not a choice.  Per frame, in this order, N = win_length, c < n_ceps:

    lm[m]  = ln(max(M[m], 2^-23))
    C[c]   = sum over m of dct[c, m] * lm[m]
    out[c] = lifter[c] * C[c]
    E      = ln(max(sum over n of e[n]^2, 2^-23))        (use_energy.  raw_energy: e = d, the frame after scale and
                                                          remove_dc_offset, BEFORE pre-emphasis and window; else e = a)
    E      = max(E, ln(energy_floor))                     (energy_floor > 0; the comparison is in the log domain, as Kaldi's;
                                                          ln(energy_floor) is taken once, in float64, and rounded to float32)
    out[0] = E                                            (use_energy: in the place of C[0], un-liftered)

    dct[0, m]   = sqrt(1 / n_mels);  dct[c, m] = sqrt(2 / n_mels) cos(pi / n_mels (m + 0.5) c),  c >= 1
    lifter[c]   = 1 + 0.5 Q sin(pi c / Q),  Q = cepstral_lifter; all ones for Q = 0

Both tables are built in float64 and rounded to float32 once, as fbank's three.  The layout is the project's,
[..., n_ceps, T']: Kaldi's matrix transposed, so `Deltas`, `MeanVar` and `SpecAugment` work behind it.

The kernel's float32 order (`mfcc_host_f32` follows the kernel).  Up to M it is fbank's.  lm is one logf.  C[c] is a chain of
fused multiply-adds in ascending m from zero; out[c] is one product.  The energy follows the mean: eight partial sums, partial
j over the taps j, j + 8 ... in ascending n, each a chain part = fma(e[n], e[n], part), added as the tree ((p0 + p1) +
(p2 + p3)) + ((p4 + p5) + (p6 + p7)); then one logf.  With u = 2^-24, fbank's dM, and [lo, hi] the interval the log of a mel
sum lies in -- lo = ln(max(M - dM, 2^-23)), hi = ln(max(M + dM, 2^-23)), each widened by 4 u (|ln| + 1) for logf -- the
half-width is w_m = max(hi_m - lm_m, lm_m - lo_m), and a float32 evaluation in that order stays within

    dC_c = |lifter_c| (sum over m of |dct[c, m]| w_m + (n_mels + 1) u sum over m of |dct[c, m] lm_m|) + u |out_c|

of the exact value (the lifter is negative where sin(pi c / Q) is below -2 / Q: cepstra 23 .. 43 at Q = 22).  The energy's
bound is the mean's carried through the squares: with fbank's e_d (raw_energy) or e_a as e_e,

    dS = sum over n of (2 |e[n]| e_e[n] + e_e[n]^2) + (1 + 2^-10) (N / 8 + 4) u sum over n of (|e[n]| + e_e[n])^2

and the half-width of the log's interval of S - dS .. S + dS as above; the clamp at ln(energy_floor) does not widen it.
`mfcc_host(..., bound=True)` returns dC, the energy's bound in line 0 with use_energy.  The bound is loose by construction --
dM is a worst case, and pre-emphasis leaves the lowest filters little power -- so the tests hold the kernel to a small multiple
of the twin's own error as well, and to the DCT of the fbank kernel's own bits, which is tight.

Input that is not finite follows IEEE arithmetic as in fbank.py: a NaN at sample i reaches exactly the frames that contain i,
there every cepstrum and the energy; every other frame is bit for bit what it is without it.

`use_energy=False` is the default here as it is torchaudio's and nearly every recipe's `mfcc.conf` (Kaldi's own binary defaults
to true; the recipes switch it off).

Out of scope: `dither`, `htk_compat`, VTLN, `use_energy` for `KaldiFbank` itself (it would change that transform's line
count), and sliding-window CMVN.

`kaldi_dct`, `kaldi_lifter`, `KaldiMfcc`, `mfcc_host` and `mfcc_host_f32` need no device.  `mfcc` is the call on device
tensors.
"""
import math

import numpy as np

from ._stageargs import _f32_finite, _fma32
from .fbank import (FLAG_REMOVE_DC, FLAG_SNIP_EDGES, FLAG_USE_POWER, FLOOR, MEAN_PARTIALS, _flag, _kaldi_fields, _KaldiFraming,
                    _row_f32, _row_f64, _rows_of, fbank_frame_index)
from .features import _chain, _int, _on_device, _Transform

FLAG_USE_ENERGY, FLAG_RAW_ENERGY = 16, 32                       # alacgpu_mfcc_device's flags beside fbank's 1, 2, 4
_U = 2.0 ** -24


def kaldi_dct(n_ceps, n_mels):
    """Kaldi's DCT-II matrix, float32 [n_ceps, n_mels], computed in float64 and rounded once: row 0 is sqrt(1 / n_mels), row
    c >= 1 is sqrt(2 / n_mels) cos(pi / n_mels (m + 0.5) c).  Its rows are orthonormal."""
    n_mels = _int("n_mels", n_mels, 1)
    n_ceps = _int("n_ceps", n_ceps, 1, n_mels)
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    c = np.arange(n_ceps, dtype=np.float64)[:, None]
    dct = math.sqrt(2.0 / n_mels) * np.cos(np.pi / n_mels * (m + 0.5) * c)
    dct[0, :] = math.sqrt(1.0 / n_mels)
    return dct.astype(np.float32)


def kaldi_lifter(n_ceps, Q):
    """Kaldi's cepstral lifter, float32 [n_ceps], computed in float64 and rounded once: 1 + 0.5 Q sin(pi c / Q); ones for
    Q = 0"""
    n_ceps = _int("n_ceps", n_ceps, 1)
    Q = _f32_finite("cepstral_lifter", Q, 0.0)
    if Q == 0.0:
        return np.ones(n_ceps, dtype=np.float32)
    return (1.0 + 0.5 * Q * np.sin(np.pi * np.arange(n_ceps, dtype=np.float64) / Q)).astype(np.float32)


class KaldiMfcc(_KaldiFraming, _Transform):
    """An immutable description of Kaldi's MFCC transform (see the module) together with its five float32 tables: fbank's
    `window` [win_length], `basis` [win_length, 2 * n_bins] and `fb` [n_filters, n_bins], `dct` [n_ceps, n_filters] and
    `lifter` [n_ceps] (read-only arrays).  The arguments are `KaldiFbank`'s without `log`, with Kaldi's MFCC defaults
    (n_mels=23 filters), and n_ceps cepstra of them, cepstral_lifter Q, use_energy (line 0 is the frame's log energy instead of
    C0), raw_energy (the energy before pre-emphasis and window) and energy_floor (0: none).  use_energy=False is the default
    here as it is torchaudio's and nearly every recipe's mfcc.conf.  The features are [..., n_ceps, T'].  The attribute
    `n_mels` is the number of output lines, n_ceps -- what `Corpus.crops`, `Deltas`, `MeanVar` and `SpecAugment` see of a
    transform; the filter count is `n_filters`.  ValueError: what `KaldiFbank` refuses, n_ceps outside 1 .. n_mels, a
    cepstral_lifter or energy_floor that is negative or not finite in float32, a use_energy or raw_energy that is not True or
    False."""

    __slots__ = ("dct", "lifter", "sample_rate", "win_length", "hop_length", "n_mels", "n_filters", "n_ceps", "n_fft", "n_bins",
                 "low_freq", "high_freq", "preemphasis", "remove_dc_offset", "window_type", "round_to_power_of_two", "snip_edges",
                 "use_power", "scale", "cepstral_lifter", "use_energy", "raw_energy", "energy_floor", "log_energy_floor")
    _TABLES = ("window", "basis", "fb", "dct", "lifter")

    def __init__(self, sample_rate, win_length=400, hop_length=160, n_mels=23, n_ceps=13, cepstral_lifter=22.0, use_energy=False,
                 raw_energy=True, energy_floor=0.0, low_freq=20.0, high_freq=0.0, preemphasis=0.97, remove_dc_offset=True,
                 window="povey", round_to_power_of_two=True, snip_edges=True, use_power=True, scale=32768.0):
        tables, fields = _kaldi_fields(sample_rate, win_length, hop_length, n_mels, low_freq, high_freq, preemphasis, window, scale,
                                       remove_dc_offset=remove_dc_offset, round_to_power_of_two=round_to_power_of_two,
                                       snip_edges=snip_edges, use_power=use_power)
        n_filters = tables[2].shape[0]
        n_ceps = _int("n_ceps", n_ceps, 1, n_filters)
        use_energy, raw_energy = _flag("use_energy", use_energy), _flag("raw_energy", raw_energy)
        Q = float(np.float32(_f32_finite("cepstral_lifter", cepstral_lifter, 0.0)))
        floor = float(np.float32(_f32_finite("energy_floor", energy_floor, 0.0)))
        self._freeze(*tables, dct=kaldi_dct(n_ceps, n_filters), lifter=kaldi_lifter(n_ceps, Q), n_mels=n_ceps, n_filters=n_filters,
                     n_ceps=n_ceps, cepstral_lifter=Q, use_energy=use_energy, raw_energy=raw_energy, energy_floor=floor,
                     log_energy_floor=float(np.float32(math.log(floor))) if floor > 0.0 else -math.inf, **fields)

    def __repr__(self):
        return (f"KaldiMfcc(sample_rate={self.sample_rate}, win_length={self.win_length}, hop_length={self.hop_length}, "
                f"n_mels={self.n_filters}, n_ceps={self.n_ceps}, cepstral_lifter={self.cepstral_lifter}, use_energy={self.use_energy}, "
                f"raw_energy={self.raw_energy}, energy_floor={self.energy_floor}, n_fft={self.n_fft}, window={self.window_type!r}, "
                f"snip_edges={self.snip_edges}, preemphasis={self.preemphasis})")

    @property
    def flags(self):
        """alacgpu_mfcc_device's flags: 1 snip_edges, 2 remove_dc_offset, 4 use_power, 16 use_energy, 32 raw_energy (with 16)"""
        return (FLAG_SNIP_EDGES * self.snip_edges | FLAG_REMOVE_DC * self.remove_dc_offset | FLAG_USE_POWER * self.use_power |
                FLAG_USE_ENERGY * self.use_energy | FLAG_RAW_ENERGY * (self.use_energy and self.raw_energy))

    def launch(self, gpu, src, rows, channels, src_stride, L, out, stream):
        """The features of src (float32 device tensor, planar [rows, channels, src_stride], the first L of a plane are signal)
        into out [rows, channels, n_ceps, frames(L)] by the AlacGpuContext `gpu`: one alacgpu_mfcc_device call on `stream`"""
        window, basis, fb, dct, lifter = self.device_tables(src.device)
        gpu.mfcc_device(src, rows, channels, src_stride, L, self.win_length, self.n_fft, self.hop_length, self.n_filters, self.n_ceps,
                        window, basis, fb, dct, lifter, self.flags, self.preemphasis, self.scale, self.energy_floor, out,
                        self.frames(L), stream=stream)


def _log_interval(v, dv):
    """(ln(max(v, floor)), the half-width of the interval a float32 logf of a value within dv of v lies in): the interval of
    tests/test_fbank.py's check_log, 4 u (|ln| + 1) for logf included"""
    mid = np.log(np.maximum(v, FLOOR))
    lo, hi = np.log(np.maximum(v - dv, FLOOR)), np.log(np.maximum(v + dv, FLOOR))
    lo, hi = lo - 4 * _U * (np.abs(lo) + 1), hi + 4 * _U * (np.abs(hi) + 1)
    return mid, np.maximum(hi - mid, mid - lo)


def mfcc_host(x, spec, bound=False):
    """The kernel's specification in numpy: x float32 [..., L], L >= 1, to float64 [..., n_ceps, T'] -- float64 arithmetic on
    the float32 input and the float32 tables, scale, preemphasis and log_energy_floor of `spec`.  bound=True: returns (out,
    dC), dC float64 like out: how far a float32 evaluation in the kernel's order may be from out (the module docstring's
    bound; with use_energy line 0 is the energy's)."""
    x, L = _rows_of(x, spec, KaldiMfcc)
    idx = fbank_frame_index(L, spec)
    T, N = idx.shape[0], spec.win_length
    dct, lifter = spec.dct.astype(np.float64), spec.lifter.astype(np.float64)
    rows = x.reshape(-1, L).astype(np.float64)
    out = np.empty((rows.shape[0], spec.n_ceps, T), dtype=np.float64)
    dC = np.empty_like(out) if bound else None
    for r, row in enumerate(rows):
        M, dM, d, a, e_d, e_a = _row_f64(row, idx, spec, bound)
        lm, w = _log_interval(M, dM if bound else 0.0)               # [T, n_filters]
        res = lifter[None, :] * (lm @ dct.T)                         # [T, n_ceps]
        if bound:
            err = np.abs(lifter)[None, :] * (w @ np.abs(dct).T + (spec.n_filters + 1) * _U * (np.abs(lm) @ np.abs(dct).T)) + _U * np.abs(res)
        if spec.use_energy:
            e, e_e = (d, e_d) if spec.raw_energy else (a, e_a)
            S = (e * e).sum(axis=1)
            dS = 0.0
            if bound:
                dS = ((2 * np.abs(e) * e_e + e_e ** 2).sum(axis=1)
                      + (1 + 2.0 ** -10) * (N / 8 + 4) * _U * ((np.abs(e) + e_e) ** 2).sum(axis=1))
            E, w_E = _log_interval(S, dS)
            res[:, 0] = np.maximum(E, spec.log_energy_floor)
            if bound:
                err[:, 0] = w_E
        out[r] = res.T
        if bound:
            dC[r] = err.T
    out = out.reshape(x.shape[:-1] + (spec.n_ceps, T))
    return (out, dC.reshape(out.shape)) if bound else out


def mfcc_host_f32(x, spec):
    """The kernel's arithmetic in numpy, one float32 operation at a time in the order the module states: x float32 [..., L] to
    float32 [..., n_ceps, T'] (the logs are numpy's float32 ones, not the device's logf).  Its distance from `mfcc_host` is
    what a correct float32 evaluation costs: the tests hold the kernel to a small multiple of that, far inside dC."""
    x, L = _rows_of(x, spec, KaldiMfcc)
    f32 = np.float32
    idx = fbank_frame_index(L, spec)
    T, N = idx.shape[0], spec.win_length
    dctT = np.ascontiguousarray(spec.dct.astype(np.float64).T)
    rows = x.reshape(-1, L)
    out = np.empty((rows.shape[0], spec.n_ceps, T), dtype=f32)
    for r, row in enumerate(rows):
        M, d, a = _row_f32(row, idx, spec)
        lm = np.log(np.maximum(M, f32(FLOOR)))                       # [T, n_filters] float32
        res = (spec.lifter[None, :] * _chain(lm, dctT)).astype(f32)  # [T, n_ceps]
        if spec.use_energy:
            e = d if spec.raw_energy else a
            part = np.zeros((T, MEAN_PARTIALS), dtype=f32)
            for n in range(N):                                       # partial n % 8 takes tap n, ascending
                part[:, n % MEAN_PARTIALS] = _fma32(e[:, n], e[:, n], part[:, n % MEAN_PARTIALS])
            while part.shape[1] > 1:                                 # neighbours first: ((p0 + p1) + (p2 + p3)) + ...
                part = part[:, 0::2] + part[:, 1::2]
            E = np.log(np.maximum(part[:, 0], f32(FLOOR)))
            res[:, 0] = np.maximum(E, f32(spec.log_energy_floor))
        out[r] = res.T
    return out.reshape(x.shape[:-1] + (spec.n_ceps, T))


# ---- on the device -------------------------------------------------------------------------------------------------------------
def mfcc(pcm, spec, lengths=None):
    """Kaldi MFCC features on the GPU: pcm float32 [..., T] on the device (as `load`, `load_batch` and `crops` return it),
    T >= 1, to float32 [..., spec.n_ceps, spec.frames(T)]; one kernel, asynchronous on the current stream.  Every row is
    transformed over its whole T.  A T that gives no frame gives an empty tensor and no launch.  lengths (a sequence or an
    integer tensor): returns (features, `fbank.fbank_lengths` of them as an int64 tensor where `lengths` was)."""
    takes = "[..., T], T >= 1"
    short = lambda T: f"pcm must be a float32 device tensor {takes}" if T < 1 else None
    return _on_device(pcm, spec, KaldiMfcc, takes, short, lengths)
