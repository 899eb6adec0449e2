"""Kaldi's pitch features behind the crops: what `compute-kaldi-pitch-feats | process-kaldi-pitch-feats` produce (Ghahremani
et al., "A pitch extraction algorithm tuned for automatic speech recognition", ICASSP 2014), three launches
(alacgpu_kaldi_pitch_device, csrc/alac_kaldi_pitch.hip): the downsampled signal with the partial sums of its mean square, the
NCCF of every frame on the lag grid, then a dense Viterbi decode along every line with the post-processing as its epilogue.
Kaldi is not at hand where this is built: the parity is with this written specification, and the deviations from Kaldi's two
tools are listed at the end.

KaldiPitch(sample_rate, frame_length_ms, frame_shift_ms, min_f0, max_f0, soft_min_f0, penalty_factor, lowpass_cutoff,
resample_freq, delta_pitch, nccf_ballast, lowpass_filter_width, upsample_filter_width, preemphasis, snip_edges, process, and
the post-processor's pitch_scale, pov_scale, pov_offset, delta_pitch_scale, normalization_left_context,
normalization_right_context, delta_window, add_pov_feature, add_normalized_log_pitch, add_delta_pitch, add_raw_log_pitch).
Derived, with fs = sample_rate and fr = resample_freq:

    win_length = floor(fs frame_length_ms / 1000), hop_length = floor(fs frame_shift_ms / 1000)      samples of the input
    window W   = floor(fr frame_length_ms / 1000), shift = floor(fr frame_shift_ms / 1000)           samples at fr (100, 40)
    lag_s      = (1 / max_f0) (1 + delta_pitch)^s while <= 1 / min_f0, s = 0 .. n_states - 1         417 states at the defaults
    first_lag  = ceil(fr (1 / max_f0 - w / (2 fr))),  last_lag = floor(fr (1 / min_f0 + w / (2 fr)))  w = upsample_filter_width: 8, 82
    N(v)       = ceil(v fr / fs)                                   the downsampled samples of a row of v samples
    frames(v)  = min(A, K):  A = 0 for v < win_length, else 1 + (v - win_length) // hop_length      the count of KaldiFbank
                             K = 0 for N(v) < W, else 1 + (N(v) - W) // shift                        Kaldi's own count

K is what compute-kaldi-pitch-feats gives.  K >= A wherever fs frame_shift_ms / 1000 is an integer, and K = A + 1 for the
rows whose last hop is all but complete (at 16 kHz: (v - 400) mod 160 in 157 .. 159, where N rounds up to a whole shift).
Kaldi's `paste-feats --length-tolerance` drops the surplus frames of the longer of two tracks; `frames` is that smaller count,
so `KaldiPitch.like(spec).frames(L) == spec.frames(L)` for every L wherever fs frame_shift_ms / 1000 is an integer.

The tables, each evaluated in float64 and rounded once to float32 (`KaldiPitch.tables`); the specification computes in float64
ON THESE FLOAT32 VALUES:

    down   P = fr / gcd(fs, fr) phases.  Output n = u P + ph reads the input from u (fs / gcd) + first_ph on, K taps: the
           indices i with |i / fs - ph / fr| <= c, c = lowpass_filter_width / (2 lowpass_cutoff), weights h(i / fs - ph / fr) / fs,
           h(t) = (sin(2 pi lowpass_cutoff t) / (pi t)) (1 + cos(2 pi lowpass_cutoff t / lowpass_filter_width)) / 2 inside |t| < c
           (2 lowpass_cutoff at t = 0), 0 outside: Kaldi's LinearResample.  Phases with fewer taps are padded with zeros behind.
           1 phase of 17 taps at 16 kHz, 40 of 45 at 44.1 kHz, 80 of 23 at 22.05 kHz; P K above 4096 is refused.
    up     per state the weights of Kaldi's ArbitraryResample from the integer lags first_lag .. last_lag onto lag_s: the lags
           j with |j / fr - lag_s| <= w / fr that exist, weights g(lag_s - j / fr) / fr with g the same function for the cutoff
           fr / 2 and w zeros; up_taps = the most taps of a state, the others padded with zero weights inside the range
    sl_s   = soft_min_f0 lag_s;   hz_s = 1 / lag_s;   factor = penalty_factor ln(1 + delta_pitch)^2
    dc_j   = j / (2 sum_{i=1}^{delta_window} i^2), j = -delta_window .. delta_window

Per row (v valid samples, zeros are read outside them), in this order:

    1.  d[n] = sum_k down[ph][k] x[u (fs / gcd) + first_ph + k], n < N(v), added in ascending k from 0
    2.  S = sum d[n], Q = sum d[n]^2 over the whole row in float64: the samples in chunks of 1024, thread j of a chunk adds
        n = 1024 c + j, + 256, + 512, + 768 in that order, the 256 threads are added as a tree of halves, the chunks in
        ascending order.  ballast = ((Q / N - (S / N)^2) W)^2 nccf_ballast in float64, rounded once to float32
    3.  frame t reads a[i] = d[t shift + i], i < W + last_lag, zeros at and behind N.  With preemphasis c != 0:
        a[i] -= c a[i - 1] for i >= 1 and a[0] -= c a[0], all from the unchanged values.  m = (sum_{i<W} a[i]) / W,
        z[i] = a[i] - m for every i (the zeros behind N too, as Kaldi does)
    4.  e1 = sum_{i<W} z[i]^2; for every lag l in first_lag .. last_lag: inner = sum_{i<W} z[i] z[i + l], e2 = sum_{i<W} z[i + l]^2,
        norm = e1 e2, pitch NCCF = inner / sqrt(norm + ballast), POV NCCF = inner / sqrt(norm), each 0 where its root is 0
    5.  both onto the lag grid: nccf[s] = sum_k up[s][k] * (its NCCF at lag up_first_s + k), ascending k from 0
    6.  the decode of the line: local[s] = (1 - n) + sl_s n with n the pitch NCCF of state s;
        f_0[s] = local_0[s];  f_t[i] = min_j (f_{t-1}[j] + (i - j)^2 factor) + local_t[i], over ALL source states j, every tie to
        the lowest j (a candidate replaces the best so far only when strictly smaller, candidates ascend); after every frame
        (frame 0 too) the least f_t is subtracted from all.  The path is walked back from the first least f of the last frame.
        Raw track: line 0 the POV NCCF at the decoded state, line 1 hz of it: compute-kaldi-pitch-feats' two columns.
    7.  the post-processing, per frame with n the raw line 0 limited to -1 .. 1 and lp = ln(line 1):
        POV feature  pov_scale ((1.0001 - n)^0.15 - 1) + pov_offset
        weight       p = 1 / (1 + exp(-r)), r = -5.2 + 5.4 exp(7.5 (|n| - 1)) + 4.8 |n| - 2 exp(-10 |n|) + 4.2 exp(20 (|n| - 1))
        normalised   pitch_scale (lp_t - (sum p_u lp_u) / (sum p_u)), u over t - left .. t + right clipped to the line's frames,
                     each window summed from its own elements in ascending u (never a difference of running sums)
        delta        delta_pitch_scale sum_j dc_j lp[clip(t + j)], ascending j, the line's first and last frame repeated
        raw log      lp
        The lines asked for, in Kaldi's order: POV feature, normalised log-pitch, delta, raw log-pitch (3 at the defaults).

The output is float32 [B, C, lines, T'], T' = frames(T); every element at and behind a row's frame count is zero, a row with
fewer samples than a frame has count 0 and runs nothing.

`kaldi_pitch_host` is the above in float64 on the float32 input.  `kaldi_pitch_host_f32` is the kernels, operation by
operation, and equals them bit for bit (fl: one float32 rounding, nothing contracted, divisions and roots correctly rounded):

    1.  acc = fma(w, x, acc) from 0                                4.  chains of fma from 0 in ascending i; e1 and the mean
    3.  fl(a[i] - fl(c a[i - 1])); the mean: lane i mod 64 adds        by 64 lanes (i mod 64, ascending) and the tree of halves;
        its elements ascending, the tree of halves, fl(sum / W)         fl(e1 e2), fl(norm + ballast), sqrt, one division
    5.  acc = fma(w, nccf, acc) from 0                             6.  fl(fl(1 - n) + fl(sl n)); fl(f[j] + fl(float((i - j)^2) factor));
    7.  log2 and exp2 are pcen.py's explicit polynomials:               fl(min + local); fl(f - least)
        lp = fl(log2(hz) LN2); x^0.15 = exp2(fl(0.15 log2(x))); exp(x) = exp2(fl(x LOG2E)); POV feature
        fl(fl(pov_scale fl(pw - 1)) + pov_offset); r = fl(fl(fl(fl(-5.2 + fl(5.4 E1)) + fl(4.8 |n|)) - fl(2 E2)) + fl(4.2 E3));
        p = fl(1 / fl(1 + exp(fl(-r)))); sums from 0: sp = fl(sp + p), sl = fl(sl + fl(p lp));
        fl(pitch_scale fl(lp - fl(sl / sp))); delta: acc = fl(acc + fl(dc_j lp)) from 0, fl(delta_pitch_scale acc)

Scaling the input by 2^k leaves the raw track bit-identical while nothing overflows or turns subnormal: norm carries the
fourth power of the scale, so for a signal of unit amplitude |k| <= 20 is safe (`test_kaldi_pitch_spec.py` checks -20 .. 20).

The bounds, u = 2^-24, gamma_k = k u / (1 - k u).  `nccf_bound(spec, info)` bounds, per frame, plane and state, how far ANY
correct float32 evaluation of steps 1 to 5 is from the specification.  With X = max |x| of the row, G the largest sum of
|down| of a phase, A = max |a| of the frame, a mean-removed sample is off by at most
    Dz = 2 (gamma_K G X (1 + |c|) + 2 u A) + gamma_{ceil(W / 64) + 8} A
(the downsampler's chain twice -- sample and mean --, the pre-emphasis, the mean's sums and its division, the subtraction).
With a1 = sqrt(e1), a2 = sqrt(e2): |d inner| <= Dz sqrt(W) (a1 + a2) + W Dz^2 + gamma_{W+1} (a1 + Dz sqrt W)(a2 + Dz sqrt W) = dI,
|d e_k| <= 2 Dz sqrt(W) a_k + W Dz^2 + gamma_{W+1} (a_k + Dz sqrt W)^2 = dE_k, |d norm| <= e1 dE2 + e2 dE1 + dE1 dE2 + u norm'
= dN, and for the quotient q = inner / sqrt(norm + ballast) (ballast itself within 2 u of the specification's):
    |d q| <= (dI + |inner| (dN + 3 u (norm + ballast)) / (2 (norm + ballast - dN'))) / sqrt(norm + ballast - dN') + 3 u |q'|
with dN' = dN + 3 u (norm + ballast), infinite where that is not below norm + ballast (a silent frame's POV NCCF: 0 / 0 is
defined as 0 only where norm is exactly 0).  The interpolation adds sum |up| dq + gamma_{up_taps} sum |up| |q|.

The decode: a normalised forward cost lies in [0, V], V = (n_states - 1)^2 factor + 2 Lmax, Lmax = 2 + 2 max sl >= |local|.
A path's float32 cost passes seven roundings per frame (three of the local cost, the transition's product, the two sums, the
subtraction), each at most u V, so its computed cost is within R = 7 T' u V (1 + 2^-20) of its float64 cost ON THE SAME
NCCF, and the float64 cost of the float32 path exceeds the float64 optimum by at most

    D(T') = 2 R = 14 T' u V (1 + 2^-20)                                                                  (`decode_bound`)

How near the decoded pitch of a pure sine of f Hz is to f (`sine_bound_cents`), to first order, with a = 2 pi f / fr the
sine's phase step at fr and lag0 = 1 / f.  With nccf_ballast 7000 the root of the pitch NCCF is the ballast's -- norm is
(frame energy)^2, the ballast 7000 (W times the row's mean square)^2 --, so the pitch NCCF is inner(lag) over a constant, and
for z = x - m, x a sine, inner(lag) = (W / 2) cos(a lag) - R(lag) / 2 - m S(lag):
    the grid      the cost is smooth at its minimum, the decoded state is the nearest: delta_pitch / 2 of the lag
    soft_min_f0   the minimum of 1 - n(lag) (1 - soft lag) lies soft / (4 pi^2 f (1 - soft / f)) of the lag below lag0
    the window    R(lag) = sum_{i<W} cos(a (2 i + lag) + 2 phase) = cos(..) sin(a W) / sin(a): a window that holds no whole or half
                  number of periods.  Its slope is at most a |sin(a W) / sin(a)|, against the cosine's curvature (W / 2) a^2:
                  |sin(a W)| / (2 pi W |sin(a)|) of the lag
    the mean      m = (sum x) / W is at most |sin(a W / 2)| / (W |sin(a / 2)|), the slope of S(lag) = sum x[i + lag] at most
                  a / |sin(a / 2)|: |sin(a W / 2)| / (pi W^2 sin(a / 2)^2) of the lag
The windowed-sinc interpolation is symmetric: it scales a cosine without moving its peak and adds nothing to first order; the
transitions cost nothing on a constant path.  The sum is 10.6 cents at 80 Hz, 18.1 at 100, 7.2 at 160, 14.3 at 250 and 11.3 at
333 Hz; a decode two grid states off is 17.3 cents off.  Measured by `test_kaldi_pitch_spec.py::test_sines_decode_within_the_bound`
on sines of 80, 100, 125, 160, 200, 250 and 333 Hz at 16 kHz, every frame inside the sine: 5.97, 0.42, 1.82, 6.18, 0.21, 6.60
and 6.53 cents at worst, 6.60 over all.

What differs from Kaldi's tools: the mean square of the ballast is that of the whole row at once (Kaldi's offline tool adds it
up as chunks arrive and recomputes the first `recompute_frame` frames); the lag grid and all tables are evaluated in float64
and rounded once (Kaldi's BaseFloat recurrence); every tie of the decode goes to the lowest source state and the minimum is
the full one (Kaldi's pruned search finds the same minimum and may break an exact tie otherwise); the frame count is the
smaller of Kaldi's and KaldiFbank's (above); log, exp and the 0.15 power are the polynomials named.  Not built, and refused or
absent: snip_edges=False, `delta_pitch_noise_stddev` (0 here), the online and latency options (`max_frames_latency`,
`frames_per_chunk`, `simulate_first_pass_online`, `recompute_frame`, `nccf_ballast_online`), `f0=` together with `vad=`,
autograd, state across calls.

The NCCF planes, the downsampled rows and the uint16 backpointers [B C, T', n_states] live in the context's scratch:
ValueError where it would pass 2^31 bytes.
"""
import math
from fractions import Fraction

import numpy as np

from ._stageargs import _device_context, _f32_finite, _fma32, _lengths_device, _lengths_host, _planes, _span, _Spec
from .pcen import _exp2_f32, _log2_f32
from .yin import _gamma, _int

_U = 2.0 ** -24
MAX_STATES, MAX_DOWN_TABLE, MAX_LDS = 1024, 4096, 65536      # ALAC_KPITCH_MAX_STATES, _MAX_DOWN, the NCCF launch's LDS in bytes
CHUNK, THREADS = 1024, 256                                   # ALAC_KPITCH_CHUNK, ALAC_KPITCH_THREADS of csrc/alac_kaldi_pitch.h
SCRATCH_MAX = 1 << 31
HEAD = 8                                                     # the scalars in front of the packed table
FLAG_PROCESS, FLAG_POV, FLAG_NORM, FLAG_DELTA, FLAG_RAW = 1, 2, 4, 8, 16
_LN2, _LOG2E = np.float32(0.6931471805599453), np.float32(1.4426950408889634)
_TABLES = {}


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, not {v!r}")
    return bool(v)


def _sinc_hann(t, cutoff, zeros):
    """Kaldi's FilterFunc on an array of times: the sinc of `cutoff` under a Hann window of `zeros` zeros to either side"""
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) < zeros / (2.0 * cutoff)
    with np.errstate(all="ignore"):
        f = np.where(t != 0, np.sin(2 * np.pi * cutoff * t) / (np.pi * np.where(t != 0, t, 1.0)), 2.0 * cutoff)
    return np.where(inside, f * 0.5 * (1.0 + np.cos(2 * np.pi * cutoff / zeros * t)), 0.0)


class KaldiPitch(_Spec):
    """An immutable description of Kaldi's pitch features (see the module).  ValueError: sample_rate or resample_freq no
    positive integer, frames without a sample, f0 limits that are not 0 < min_f0 < max_f0, delta_pitch not above 0, a cutoff at
    or above half the lower rate, filter widths below 1, more than 1024 states, a rate whose polyphase table passes 4096
    weights, a frame too long for the launch, snip_edges=False, process=True without a line, a number not finite in float32."""

    __slots__ = ("sample_rate", "frame_length_ms", "frame_shift_ms", "min_f0", "max_f0", "soft_min_f0", "penalty_factor", "lowpass_cutoff",
                 "resample_freq", "delta_pitch", "nccf_ballast", "lowpass_filter_width", "upsample_filter_width", "preemphasis", "snip_edges",
                 "process", "pitch_scale", "pov_scale", "pov_offset", "delta_pitch_scale", "normalization_left_context",
                 "normalization_right_context", "delta_window", "add_pov_feature", "add_normalized_log_pitch", "add_delta_pitch",
                 "add_raw_log_pitch")

    def __init__(self, sample_rate, frame_length_ms=25, frame_shift_ms=10, min_f0=50, max_f0=400, soft_min_f0=10, penalty_factor=0.1,
                 lowpass_cutoff=1000, resample_freq=4000, delta_pitch=0.005, nccf_ballast=7000, lowpass_filter_width=1,
                 upsample_filter_width=5, preemphasis=0.0, snip_edges=True, process=True, pitch_scale=2, pov_scale=2, pov_offset=0,
                 delta_pitch_scale=10, normalization_left_context=75, normalization_right_context=75, delta_window=2,
                 add_pov_feature=True, add_normalized_log_pitch=True, add_delta_pitch=True, add_raw_log_pitch=False):
        s = object.__setattr__
        s(self, "sample_rate", _int("sample_rate", sample_rate, 1, (1 << 31) - 1))
        s(self, "resample_freq", _int("resample_freq", resample_freq, 1, self.sample_rate))
        for name, v in (("frame_length_ms", frame_length_ms), ("frame_shift_ms", frame_shift_ms), ("min_f0", min_f0), ("max_f0", max_f0),
                        ("soft_min_f0", soft_min_f0), ("penalty_factor", penalty_factor), ("lowpass_cutoff", lowpass_cutoff),
                        ("delta_pitch", delta_pitch), ("nccf_ballast", nccf_ballast), ("preemphasis", preemphasis),
                        ("pitch_scale", pitch_scale), ("pov_scale", pov_scale), ("pov_offset", pov_offset),
                        ("delta_pitch_scale", delta_pitch_scale)):
            s(self, name, _f32_finite(name, v))
        s(self, "lowpass_filter_width", _int("lowpass_filter_width", lowpass_filter_width, 1, 64))
        s(self, "upsample_filter_width", _int("upsample_filter_width", upsample_filter_width, 1, 64))
        s(self, "normalization_left_context", _int("normalization_left_context", normalization_left_context, 0, (1 << 20)))
        s(self, "normalization_right_context", _int("normalization_right_context", normalization_right_context, 0, (1 << 20)))
        s(self, "delta_window", _int("delta_window", delta_window, 1, 64))
        for name, v in (("snip_edges", snip_edges), ("process", process), ("add_pov_feature", add_pov_feature),
                        ("add_normalized_log_pitch", add_normalized_log_pitch), ("add_delta_pitch", add_delta_pitch),
                        ("add_raw_log_pitch", add_raw_log_pitch)):
            s(self, name, _flag(name, v))
        if not self.snip_edges:
            raise ValueError("snip_edges=False is not built: Kaldi's pitch then centres its frames and counts them otherwise")
        if not (self.frame_length_ms > 0 and self.frame_shift_ms > 0) or self.hop_length < 1 or self.shift < 1 or self.window < 2:
            raise ValueError(f"frame_length_ms {frame_length_ms!r} and frame_shift_ms {frame_shift_ms!r} must leave whole samples at "
                             f"{self.sample_rate} and {self.resample_freq} Hz")
        if not 0.0 < self.min_f0 < self.max_f0:
            raise ValueError(f"min_f0 and max_f0 must be 0 < min_f0 < max_f0, not {min_f0!r} and {max_f0!r}")
        if not self.delta_pitch > 0.0 or not self.soft_min_f0 >= 0.0 or not self.penalty_factor >= 0.0 or not self.nccf_ballast >= 0.0:
            raise ValueError("delta_pitch must be above 0; soft_min_f0, penalty_factor and nccf_ballast at least 0")
        if not 0.0 < self.lowpass_cutoff < 0.5 * self.resample_freq:
            raise ValueError(f"lowpass_cutoff must be in (0, resample_freq / 2), not {lowpass_cutoff!r}")
        if not 0.0 <= self.preemphasis <= 1.0:
            raise ValueError(f"preemphasis must be in [0, 1], not {preemphasis!r}")
        n = self._count_states()
        if n > MAX_STATES:
            raise ValueError(f"min_f0 {min_f0!r}, max_f0 {max_f0!r} at delta_pitch {delta_pitch!r}: {n} states are above {MAX_STATES}")
        if self.first_lag < 1 or self.last_lag <= self.first_lag:
            raise ValueError(f"max_f0 {max_f0!r} at {self.resample_freq} Hz: the integer lags {self.first_lag} .. {self.last_lag} leave nothing")
        P, K = self.phases, self._down()[1].shape[1]
        if P * K > MAX_DOWN_TABLE:
            raise ValueError(f"{self.sample_rate} Hz to {self.resample_freq} Hz: {P} phases of {K} taps are above {MAX_DOWN_TABLE} weights")
        if self.lds_bytes > MAX_LDS:
            raise ValueError(f"frames of {self.span} samples and {self.n_lags} lags: {self.lds_bytes} bytes of LDS are above {MAX_LDS}")
        if self.process and self.lines == 0:
            raise ValueError("process=True needs one of add_pov_feature, add_normalized_log_pitch, add_delta_pitch, add_raw_log_pitch")

    @classmethod
    def like(cls, spec, **kw):
        """The KaldiPitch beside `spec`, a fbank.KaldiFbank or a mfcc.KaldiMfcc with snip_edges: its rate and its shift.  The
        frame length stays frame_length_ms (25 unless given in kw): with spec's window of that length -- Kaldi's default, 400
        samples at 16 kHz -- `frames` is spec's for every L.  kw: the other arguments of `KaldiPitch`."""
        from .fbank import _KaldiFraming

        if not isinstance(spec, _KaldiFraming):
            raise ValueError(f"spec must be a fbank.KaldiFbank or a mfcc.KaldiMfcc, not {spec!r}")
        if not spec.snip_edges:
            raise ValueError("a Kaldi transform with snip_edges=False reflects its last frames: no KaldiPitch has its frame count")
        kw.setdefault("frame_shift_ms", spec.hop_length * 1000.0 / spec.sample_rate)
        return cls(spec.sample_rate, **kw)

    # ---- the framing -------------------------------------------------------------------------------------------------------
    win_length = property(lambda self: math.floor(self.sample_rate * self.frame_length_ms / 1000.0 + 1e-6))
    hop_length = property(lambda self: math.floor(self.sample_rate * self.frame_shift_ms / 1000.0 + 1e-6))
    window = property(lambda self: math.floor(self.resample_freq * self.frame_length_ms / 1000.0 + 1e-6))
    shift = property(lambda self: math.floor(self.resample_freq * self.frame_shift_ms / 1000.0 + 1e-6))

    def samples(self, L):
        """N(L): the downsampled samples of a row of L samples (numpy arrays too)"""
        return (np.asarray(L, dtype=np.int64) * self.resample_freq + self.sample_rate - 1) // self.sample_rate

    def frames(self, L):
        """T' of a row of L samples (numpy arrays too): the smaller of KaldiFbank's count and Kaldi's own (see the module)"""
        L = np.asarray(L, dtype=np.int64)
        N = self.samples(L)
        a = np.where(L < self.win_length, 0, 1 + (L - self.win_length) // self.hop_length)
        k = np.where(N < self.window, 0, 1 + (N - self.window) // self.shift)
        T = np.minimum(a, k)
        return int(T) if np.ndim(T) == 0 else T

    @property
    def min_frames(self):
        """The shortest row that has a frame"""
        return max(self.win_length, (self.window - 1) * self.sample_rate // self.resample_freq + 1)

    def short(self, L):
        return f"num_frames {L}: a row of fewer than {self.min_frames} samples has no pitch frame"

    def lengths(self, lengths):
        """The frame count `frames` gives each length, -1 where a length is -1: an int64 torch tensor on the device of
        `lengths` for a tensor, an int64 numpy array for anything else"""
        try:
            import torch
        except ImportError:
            torch = None
        if torch is not None and isinstance(lengths, torch.Tensor):
            if lengths.dtype.is_floating_point:
                raise ValueError("lengths must be integers")
            lens = lengths.to(torch.int64)
            pos = lens.clamp(min=0)
            N = torch.div(pos * self.resample_freq + self.sample_rate - 1, self.sample_rate, rounding_mode="floor")
            a = torch.where(pos < self.win_length, torch.zeros_like(pos), 1 + torch.div(pos - self.win_length, self.hop_length, rounding_mode="floor"))
            k = torch.where(N < self.window, torch.zeros_like(pos), 1 + torch.div(N - self.window, self.shift, rounding_mode="floor"))
            return torch.where(lens >= 0, torch.minimum(a, k), torch.full_like(lens, -1))
        lens = np.asarray(lengths)
        if lens.dtype.kind not in "iu":
            raise ValueError("lengths must be integers")
        lens = lens.astype(np.int64)
        return np.where(lens >= 0, np.asarray(self.frames(np.maximum(lens, 0)), dtype=np.int64), -1)

    # ---- the grid and the tables -------------------------------------------------------------------------------------------
    def _count_states(self):
        return math.floor(math.log(self.max_f0 / self.min_f0) / math.log1p(self.delta_pitch) + 1e-9) + 1

    @property
    def n_states(self):
        return len(self.lags())

    def lags(self):
        """lag_s in seconds, float64"""
        n = self._count_states()
        lag = (1.0 / self.max_f0) * (1.0 + self.delta_pitch) ** np.arange(n + 1)
        return lag[lag <= 1.0 / self.min_f0 * (1.0 + 1e-12)][:n + 1]

    @property
    def first_lag(self):
        return math.ceil(self.resample_freq * (1.0 / self.max_f0 - self.upsample_filter_width / (2.0 * self.resample_freq)) - 1e-9)

    @property
    def last_lag(self):
        return math.floor(self.resample_freq * (1.0 / self.min_f0 + self.upsample_filter_width / (2.0 * self.resample_freq)) + 1e-9)

    n_lags = property(lambda self: self.last_lag - self.first_lag + 1)
    span = property(lambda self: self.window + self.last_lag)                       # the samples a frame reads at fr
    phases = property(lambda self: self.resample_freq // math.gcd(self.sample_rate, self.resample_freq))
    in_per_unit = property(lambda self: self.sample_rate // math.gcd(self.sample_rate, self.resample_freq))
    lds_bytes = property(lambda self: 4 * (THREADS // 64) * (self.span + 2 * self.n_lags))

    @property
    def flags(self):
        if not self.process:
            return 0
        return (FLAG_PROCESS | FLAG_POV * self.add_pov_feature | FLAG_NORM * self.add_normalized_log_pitch |
                FLAG_DELTA * self.add_delta_pitch | FLAG_RAW * self.add_raw_log_pitch)

    @property
    def lines(self):
        if not self.process:
            return 2
        return self.add_pov_feature + self.add_normalized_log_pitch + self.add_delta_pitch + self.add_raw_log_pitch

    def _down(self):
        """(first [P] int64, weights [P, K] float64) of the downsampler"""
        fs, fr, c, z = self.sample_rate, self.resample_freq, self.lowpass_cutoff, self.lowpass_filter_width
        half = Fraction(z) / (2 * Fraction(c))
        rows = []
        for ph in range(self.phases):
            t = Fraction(ph, fr)
            lo, hi = math.ceil((t - half) * fs), math.floor((t + half) * fs)
            i = np.arange(lo, hi + 1)
            rows.append((lo, _sinc_hann(i / fs - ph / fr, c, z) / fs))
        K = max(len(w) for _, w in rows)
        W = np.zeros((len(rows), K))
        for r, (_, w) in enumerate(rows):
            W[r, :len(w)] = w
        return np.asarray([lo for lo, _ in rows], dtype=np.int64), W

    def _up(self):
        """(first [S] int64 -- an index into the integer lags --, weights [S, K] float64) of the interpolation"""
        fr, z, n = float(self.resample_freq), self.upsample_filter_width, self.n_lags
        t = self.lags() - self.first_lag / fr
        lo = np.maximum(np.ceil(fr * (t - z / fr) - 1e-9).astype(np.int64), 0)
        hi = np.minimum(np.floor(fr * (t + z / fr) + 1e-9).astype(np.int64), n - 1)
        K = int(min(max(hi - lo + 1), n))
        first = np.minimum(lo, n - K)
        j = first[:, None] + np.arange(K)[None, :]
        w = _sinc_hann(t[:, None] - j / fr, fr / 2.0, z) / fr
        return first, np.where((j >= lo[:, None]) & (j <= hi[:, None]), w, 0.0)

    def tables(self):
        """The float32 tables of the module by name (the firsts as int64), each from float64 and rounded once"""
        f32 = np.float32
        d0, dw = self._down()
        u0, uw = self._up()
        lag = self.lags()
        w = self.delta_window
        head = np.zeros(HEAD)
        head[:7] = (self.penalty_factor * math.log1p(self.delta_pitch) ** 2, self.preemphasis, self.nccf_ballast, self.pitch_scale,
                    self.pov_scale, self.pov_offset, self.delta_pitch_scale)
        return dict(head=head.astype(f32), down_first=d0, down=dw.astype(f32), up_first=u0, up=uw.astype(f32),
                    sl=(self.soft_min_f0 * lag).astype(f32), hz=(1.0 / lag).astype(f32),
                    dc=(np.arange(-w, w + 1) / (2.0 * sum(i * i for i in range(1, w + 1)))).astype(f32))

    def table(self):
        """The tables packed as alac_kpitch_tables_at (csrc/alac_kaldi_pitch.h) reads them: alacgpu_kaldi_pitch_device's d_table.
        The firsts are stored as float32 (small integers, exact)."""
        t = self.tables()
        return np.concatenate([t["head"], t["down_first"].astype(np.float32), t["down"].ravel(), t["up_first"].astype(np.float32),
                               t["up"].ravel(), t["sl"], t["hz"], t["dc"]]).astype(np.float32)


# ---- the bounds ----------------------------------------------------------------------------------------------------------------
def decode_bound(spec, frames):
    """D(T') of the module"""
    t = spec.tables()
    Lmax = 2.0 + 2.0 * float(np.max(np.abs(t["sl"])))
    V = (spec.n_states - 1) ** 2 * float(t["head"][0]) + 2.0 * Lmax
    return 14.0 * frames * _U * V * (1.0 + 2.0 ** -20)


def sine_bound_cents(spec, f):
    """How many cents the decoded pitch of a pure sine of f Hz may be from f, to first order (the module docstring): the grid,
    soft_min_f0, the window's ripple and the mean's"""
    s, W = spec.soft_min_f0, spec.window
    a = 2.0 * math.pi * f / spec.resample_freq
    rel = (spec.delta_pitch / 2.0 + s / (4.0 * math.pi ** 2 * f * (1.0 - s / f))
           + abs(math.sin(a * W)) / (2.0 * math.pi * W * abs(math.sin(a)))
           + abs(math.sin(a * W / 2.0)) / (math.pi * W * W * math.sin(a / 2.0) ** 2))
    return 1200.0 * math.log2(1.0 + rel)


def nccf_bound(spec, info):
    """The module's bound on both NCCF planes [B, C, 2, T', n_states] of any correct float32 evaluation, from the `info` of
    `kaldi_pitch_host(..., details=True)`; infinite where a root's argument may reach 0"""
    t = {k: v.astype(np.float64) for k, v in spec.tables().items()}
    W, K = spec.window, t["down"].shape[1]
    G = float(np.max(np.sum(np.abs(t["down"]), axis=1)))
    c = abs(float(t["head"][1]))
    X, A = info["x_max"][..., None, None], info["a_max"][..., None]                # [B, C, 1, 1], [B, C, T', 1]
    Dz = 2.0 * (_gamma(K) * G * X * (1.0 + c) + 2 * _U * A) + _gamma((W + 63) // 64 + 8) * A
    rW, g = math.sqrt(W), _gamma(W + 1)
    e1, e2, inner = info["e1"][..., None], info["e2"], info["inner"]
    a1, a2 = np.sqrt(e1), np.sqrt(e2)
    dI = Dz * rW * (a1 + a2) + W * Dz ** 2 + g * (a1 + Dz * rW) * (a2 + Dz * rW)
    dE1 = 2 * Dz * rW * a1 + W * Dz ** 2 + g * (a1 + Dz * rW) ** 2
    dE2 = 2 * Dz * rW * a2 + W * Dz ** 2 + g * (a2 + Dz * rW) ** 2
    norm = e1 * e2
    dN = e1 * dE2 + e2 * dE1 + dE1 * dE2 + _U * (norm + e1 * dE2 + e2 * dE1 + dE1 * dE2)
    out = []
    up0, up = t["up_first"].astype(np.int64), np.abs(t["up"])
    idx = up0[:, None] + np.arange(up.shape[1])[None, :]
    for ballast, q in ((info["ballast"][..., None, None], info["lag_pitch"]), (0.0, info["lag_pov"])):
        den = norm + ballast
        dD = dN + 3 * _U * den
        with np.errstate(all="ignore"):
            ok = dD < den
            room = np.where(ok, den - dD, 1.0)
            dq = np.where(ok, (dI + np.abs(inner) * dD / (2 * room)) / np.sqrt(room) + 3 * _U * (np.abs(q) + 1.0), np.inf)
            dq = np.where((den == 0) & (Dz == 0), 0.0, dq)                         # (silence is silence in every evaluation)
        with np.errstate(all="ignore"):
            spread = np.sum(np.where(up > 0, up * dq[..., idx], 0.0), axis=-1)
        out.append(spread + _gamma(up.shape[1]) * np.sum(up * np.abs(q)[..., idx], axis=-1))
    return np.stack(out, axis=2)


# ---- steps 1 to 5 --------------------------------------------------------------------------------------------------------------
def _mac(w, x, acc, f):
    return _fma32(w, x, acc) if f is np.float32 else w * x + acc


def _downsample(row, v, spec, T, f):
    """Step 1 on one row: d [N(v)] of dtype f"""
    N = int(spec.samples(v))
    n = np.arange(N, dtype=np.int64)
    u, ph = n // spec.phases, n % spec.phases
    base = u * spec.in_per_unit + T["down_first"][ph]
    acc = np.zeros(N, dtype=f)
    for k in range(T["down"].shape[1]):
        i = base + k
        x = np.where((i >= 0) & (i < v), row[np.clip(i, 0, max(len(row) - 1, 0))] if len(row) else 0, 0).astype(f)
        acc = _mac(T["down"][ph, k].astype(f), x, acc, f)
    return acc


def _row_sums(d):
    """Step 2: (S, Q) of d in float64, in the module's order"""
    S = Q = 0.0
    d = d.astype(np.float64)
    for c0 in range(0, len(d), CHUNK):
        seg = np.zeros(CHUNK)
        seg[:min(CHUNK, len(d) - c0)] = d[c0:c0 + CHUNK]
        seg = seg.reshape(CHUNK // THREADS, THREADS)
        s, q = np.zeros(THREADS), np.zeros(THREADS)
        for j in range(CHUNK // THREADS):
            s, q = s + seg[j], q + seg[j] * seg[j]
        h = THREADS // 2
        while h >= 1:
            s, q = s[:h] + s[h:2 * h], q[:h] + q[h:2 * h]
            h //= 2
        S, Q = S + s[0], Q + q[0]
    return S, Q


def _ballast(d, spec, T):
    if len(d) == 0:
        return 0.0
    S, Q = _row_sums(d)
    N = float(len(d))
    mean = S / N
    b = (Q / N - mean * mean) * float(spec.window)
    return b * b * float(T["head"][2])


def _lane_sum(terms, f, square):
    """terms [F, W] added (squared first with `square`, by fma) by 64 lanes, element i in lane i % 64 ascending, then the tree of
    halves"""
    F, W = terms.shape
    J = (W + 63) // 64
    pad = np.zeros((F, J * 64), dtype=f)
    pad[:, :W] = terms
    pad = pad.reshape(F, J, 64)
    part = np.zeros((F, 64), dtype=f)
    for j in range(J):
        part = _mac(pad[:, j], pad[:, j], part, f) if square else (part + pad[:, j]).astype(f)
    h = 32
    while h >= 1:
        part = (part[:, :h] + part[:, h:2 * h]).astype(f)
        h //= 2
    return part[:, 0]


def _nccf(d, count, ballast, spec, T, f):
    """Steps 3 to 5 on the downsampled row d for its first `count` frames: (nccf [2, count, n_states], details)"""
    W, L0, L1, S = spec.window, spec.first_lag, spec.last_lag, spec.n_states
    g = np.arange(count, dtype=np.int64)[:, None] * spec.shift + np.arange(spec.span, dtype=np.int64)[None, :]
    a = np.where(g < len(d), d[np.clip(g, 0, max(len(d) - 1, 0))] if len(d) else 0, 0).astype(f)
    c = f(T["head"][1])
    with np.errstate(all="ignore"):
        if c != 0:
            prev = np.concatenate([a[:, :1], a[:, :-1]], axis=1)
            a = (a - (c * prev).astype(f)).astype(f)
        m = (_lane_sum(a[:, :W], f, False) / f(W)).astype(f)
        z = (a - m[:, None]).astype(f)
        e1 = _lane_sum(z[:, :W], f, True)
        inner = np.zeros((count, spec.n_lags), dtype=f)
        e2 = np.zeros((count, spec.n_lags), dtype=f)
        lag = np.arange(L0, L1 + 1)
        for i in range(W):
            zl = z[:, i + lag]
            inner = _mac(z[:, i:i + 1], zl, inner, f)
            e2 = _mac(zl, zl, e2, f)
        norm = (e1[:, None] * e2).astype(f)
        dp, dv = np.sqrt((norm + f(ballast)).astype(f)).astype(f), np.sqrt(norm).astype(f)
        qp = np.where(dp != 0, inner / np.where(dp != 0, dp, f(1)), f(0)).astype(f)
        qv = np.where(dv != 0, inner / np.where(dv != 0, dv, f(1)), f(0)).astype(f)
        out = np.zeros((2, count, S), dtype=f)
        up0, up = T["up_first"], T["up"].astype(f)
        for k in range(up.shape[1]):
            out[0] = _mac(up[None, :, k], qp[:, up0 + k], out[0], f)
            out[1] = _mac(up[None, :, k], qv[:, up0 + k], out[1], f)
    return out, dict(e1=e1, e2=e2, inner=inner, lag_pitch=qp, lag_pov=qv, a_max=np.max(np.abs(a), axis=1) if count else np.zeros(0))


# ---- the decode ----------------------------------------------------------------------------------------------------------------
def _costs(spec, T, f):
    i = np.arange(spec.n_states)
    d2 = ((i[:, None] - i[None, :]) ** 2).astype(f)                                # [target, source]
    return (d2 * f(T["head"][0])).astype(f)


def _local(n, T, f):
    with np.errstate(all="ignore"):
        return ((f(1.0) - n).astype(f) + (T["sl"].astype(f) * n).astype(f)).astype(f)


def _decode_line(nccf, count, spec, T, f, cost):
    """Step 6 on nccf [2, T', S] of dtype f for a line of `count` frames: the states [count]"""
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    back = np.zeros((count, spec.n_states), dtype=np.int64)
    with np.errstate(all="ignore"):
        fwd = _local(nccf[0, 0], T, f)
        fwd = (fwd - fwd.min()).astype(f)
        for t in range(1, count):
            cand = (fwd[None, :] + cost).astype(f)
            back[t] = np.argmin(cand, axis=1)
            fwd = (cand[np.arange(len(fwd)), back[t]] + _local(nccf[0, t], T, f)).astype(f)
            fwd = (fwd - fwd.min()).astype(f)
    s = int(np.argmin(fwd))
    path = np.zeros(count, dtype=np.int64)
    for t in range(count - 1, -1, -1):
        path[t] = s
        s = int(back[t, s])
    return path


def _raw_of(nccf, path, T, f):
    raw = np.zeros((2, nccf.shape[1]), dtype=f)
    at = np.arange(len(path))
    raw[0, :len(path)] = nccf[1, at, path]
    raw[1, :len(path)] = T["hz"].astype(f)[path]
    return raw


def path_cost(nccf, states, spec, frame_counts=None):
    """The float64 cost of the paths `states` [B, C, T'] on nccf [B, C, 2, T', n_states] (the tables' float32 values, float64
    arithmetic, no normalisation): sum of the local costs and the transitions; 0 for a line without frames"""
    nccf, st = np.asarray(nccf, dtype=np.float64), np.asarray(states)
    B, C = nccf.shape[:2]
    counts = _lengths_host("frame_counts", frame_counts, B, nccf.shape[3])
    T = spec.tables()
    sl, factor = T["sl"].astype(np.float64), float(T["head"][0])
    out = np.zeros((B, C))
    for b in range(B):
        for c in range(C):
            p = st[b, c, :counts[b]].astype(np.int64)
            n = nccf[b, c, 0, np.arange(len(p)), p]
            out[b, c] = np.sum((1.0 - n) + sl[p] * n) + factor * np.sum(np.diff(p).astype(np.float64) ** 2)
    return out


# ---- the post-processing -------------------------------------------------------------------------------------------------------
def _exp(x, f):
    return _exp2_f32((x * _LOG2E).astype(f)) if f is np.float32 else np.exp(x)


def _process_line(raw, count, spec, T, f):
    """Step 7 on raw [2, T'] of dtype f for a line of `count` frames: [lines, T'] of dtype f"""
    out = np.zeros((spec.lines, raw.shape[1]), dtype=f)
    if count == 0:
        return out
    h = T["head"].astype(f)
    with np.errstate(all="ignore"):
        n = raw[0, :count]
        n = np.where(n < f(-1), f(-1), np.where(n > f(1), f(1), n)).astype(f)
        hz = raw[1, :count]
        if f is np.float32:
            lp = (_log2_f32(hz) * _LN2).astype(f)
            pw = _exp2_f32((f(0.15) * _log2_f32((f(1.0001) - n).astype(f))).astype(f))
        else:
            lp, pw = np.log(hz), (f(np.float32(1.0001)) - n) ** f(np.float32(0.15))
        povf = ((h[4] * (pw - f(1)).astype(f)).astype(f) + h[5]).astype(f)
        nd = np.abs(n)
        k = lambda v: f(np.float32(v))
        m1 = (nd - f(1)).astype(f)
        e1 = (k(5.4) * _exp((k(7.5) * m1).astype(f), f)).astype(f)
        e2 = (k(2.0) * _exp((k(-10.0) * nd).astype(f), f)).astype(f)
        e3 = (k(4.2) * _exp((k(20.0) * m1).astype(f), f)).astype(f)
        r = ((((k(-5.2) + e1).astype(f) + (k(4.8) * nd).astype(f)).astype(f) - e2).astype(f) + e3).astype(f)
        p = (f(1) / (f(1) + _exp((-r).astype(f), f)).astype(f)).astype(f)
        plp = (p * lp).astype(f)
        norm = np.zeros(count, dtype=f)
        left, right = spec.normalization_left_context, spec.normalization_right_context
        sp, sl = np.zeros(count, dtype=f), np.zeros(count, dtype=f)
        t = np.arange(count)
        for o in range(-left, right + 1):                       # ascending u = t + o; a u outside the line adds nothing
            u = t + o
            ok = (u >= 0) & (u < count)
            uc = np.clip(u, 0, count - 1)
            sp = np.where(ok, (sp + p[uc]).astype(f), sp)
            sl = np.where(ok, (sl + plp[uc]).astype(f), sl)
        norm = (h[3] * (lp - (sl / sp).astype(f)).astype(f)).astype(f)
        acc = np.zeros(count, dtype=f)
        dc = T["dc"].astype(f)
        w = spec.delta_window
        for j in range(-w, w + 1):
            acc = (acc + (dc[j + w] * lp[np.clip(t + j, 0, count - 1)]).astype(f)).astype(f)
        delta = (h[6] * acc).astype(f)
    line = 0
    for on, v in ((spec.add_pov_feature, povf), (spec.add_normalized_log_pitch, norm), (spec.add_delta_pitch, delta),
                  (spec.add_raw_log_pitch, lp)):
        if on:
            out[line, :count] = v
            line += 1
    return out


# ---- the host functions --------------------------------------------------------------------------------------------------------
def _spec_ok(spec):
    if not isinstance(spec, KaldiPitch):
        raise ValueError(f"spec must be a KaldiPitch, not {spec!r}")


def _host_args(x, spec, lengths):
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim not in (2, 3):
        raise ValueError(f"x must be float32 [B, C, T] or [B, T], not {x.dtype} {x.shape}")
    _spec_ok(spec)
    x3 = x if x.ndim == 3 else x[:, None, :]
    return x3, x.ndim == 3, _lengths_host("lengths", lengths, x.shape[0], x.shape[-1])


def _host(x, spec, lengths, f, details, upto):
    x3, had_c, lens = _host_args(x, spec, lengths)
    B, C, Tx = x3.shape
    S, nf = spec.n_states, int(spec.frames(Tx))
    T = spec.tables()
    cost = _costs(spec, T, f)
    nccf = np.zeros((B, C, 2, nf, S), dtype=f)
    raw = np.zeros((B, C, 2, nf), dtype=f)
    y = np.zeros((B, C, spec.lines, nf), dtype=f)
    states = np.full((B, C, nf), -1, dtype=np.int32)
    counts = np.minimum(np.asarray(spec.frames(lens), dtype=np.int64).reshape(B), nf)
    info = dict(e1=np.zeros((B, C, nf)), e2=np.zeros((B, C, nf, spec.n_lags)), inner=np.zeros((B, C, nf, spec.n_lags)),
                lag_pitch=np.zeros((B, C, nf, spec.n_lags)), lag_pov=np.zeros((B, C, nf, spec.n_lags)), a_max=np.zeros((B, C, nf)),
                x_max=np.zeros((B, C)), ballast=np.zeros((B, C)))
    for b in range(B):
        v, count = int(lens[b]), int(counts[b])
        for c in range(C):
            if count == 0:
                continue
            d = _downsample(x3[b, c], v, spec, T, f)
            ballast = _ballast(d, spec, T)
            if f is np.float32:
                ballast = np.float32(ballast)
            nccf[b, c, :, :count], det = _nccf(d, count, ballast, spec, T, f)
            if details:
                for k, val in det.items():
                    info[k][b, c, :count] = val
                info["x_max"][b, c] = float(np.max(np.abs(x3[b, c, :v]))) if v else 0.0
                info["ballast"][b, c] = float(ballast)
            if upto == "nccf":
                continue
            path = _decode_line(nccf[b, c], count, spec, T, f, cost)
            states[b, c, :count] = path
            raw[b, c] = _raw_of(nccf[b, c], path, T, f)
            y[b, c] = _process_line(raw[b, c], count, spec, T, f) if spec.process else raw[b, c]
    shape = (B, C) if had_c else (B,)
    res = nccf.reshape(shape + nccf.shape[2:]) if upto == "nccf" else y.reshape(shape + y.shape[2:])
    if not details:
        return res
    info.update(nccf=nccf, raw=raw, states=states, frame_counts=counts)
    return res, info


def kaldi_pitch_host(x, spec, lengths=None, details=False):
    """The specification in numpy: float64 [B, C, lines, T'] ([B, lines, T'] for x [B, T]) from x float32, float64 arithmetic
    on the float32 input and the float32 tables.  lengths: [B] integers (below 0 counts as 0, above T as T); default: T.
    details=True: returns (y, info), info a dict of `nccf` [B, C, 2, T', n_states], `raw` [B, C, 2, T'], `states` int32
    [B, C, T'] (-1 behind a row's frames), `frame_counts` [B] and what `nccf_bound` reads."""
    return _host(x, spec, lengths, np.float64, details, "all")


def kaldi_pitch_host_f32(x, spec, lengths=None, details=False):
    """The kernels' arithmetic in numpy, bit for bit: float32 [B, C, lines, T']; details as for `kaldi_pitch_host`"""
    return _host(x, spec, lengths, np.float32, details, "all")


def kaldi_pitch_nccf_host(x, spec, lengths=None, f32=False):
    """Steps 1 to 5 alone: the two NCCF planes on the lag grid [B, C, 2, T', n_states], float64 or (f32) the kernels' float32"""
    return _host(x, spec, lengths, np.float32 if f32 else np.float64, False, "nccf")


def _lines_args(a, name, spec, frame_counts, inner):
    a = np.asarray(a)
    _spec_ok(spec)
    if a.ndim != 2 + len(inner) or tuple(a.shape[2:3] + a.shape[4:]) != tuple(inner[:1] + inner[2:]):
        raise ValueError(f"{name} must be [B, C, {', '.join(str(i) for i in inner)}], not {a.shape}")
    return a, _lengths_host("frame_counts", frame_counts, a.shape[0], a.shape[3])


def kaldi_pitch_decode_host(nccf, spec, frame_counts=None, f32=False, states=False):
    """The decode alone in numpy: nccf [B, C, 2, T', n_states] to the raw track [B, C, 2, T'] (zeros at and behind a row's
    frame_counts [B], default T'); states=True: (raw, int32 states [B, C, T'], -1 behind the count).  f32: the kernel's
    float32 recursion, bit for bit; else float64."""
    f = np.float32 if f32 else np.float64
    nccf, counts = _lines_args(nccf, "nccf", spec, frame_counts, (2, "T'", spec.n_states))
    nccf = nccf.astype(f)
    B, C, _, nf, _ = nccf.shape
    T = spec.tables()
    cost = _costs(spec, T, f)
    raw = np.zeros((B, C, 2, nf), dtype=f)
    st = np.full((B, C, nf), -1, dtype=np.int32)
    for b in range(B):
        for c in range(C):
            path = _decode_line(nccf[b, c], int(counts[b]), spec, T, f, cost)
            st[b, c, :len(path)] = path
            raw[b, c] = _raw_of(nccf[b, c], path, T, f)
    return (raw, st) if states else raw


def kaldi_pitch_process_host(raw, spec, frame_counts=None, f32=False):
    """The post-processing alone in numpy: raw [B, C, 2, T'] (the POV NCCF, the pitch in Hz above 0) to [B, C, lines, T']"""
    f = np.float32 if f32 else np.float64
    raw, counts = _lines_args(raw, "raw", spec, frame_counts, (2, "T'"))
    if not spec.process:
        raise ValueError("spec.process is False: there is nothing to post-process")
    raw = raw.astype(f)
    T = spec.tables()
    B, C = raw.shape[:2]
    y = np.zeros((B, C, spec.lines, raw.shape[3]), dtype=f)
    for b in range(B):
        for c in range(C):
            y[b, c] = _process_line(raw[b, c], int(counts[b]), spec, T, f)
    return y


# ---- on the device -------------------------------------------------------------------------------------------------------------
def _table_device(spec, device):
    import torch

    key = (spec, device.index if device.index is not None else torch.cuda.current_device())
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) >= 64:
            _TABLES.pop(next(iter(_TABLES)))
        t = _TABLES[key] = torch.from_numpy(spec.table()).to(device)
    return t


def _scratch_bytes(spec, planes, T, frames):
    """What stage 0 keeps in the context's scratch (alac_kpitch_scratch of csrc/alac_kaldi_pitch.h)"""
    N = int(spec.samples(T))
    chunks = (N + CHUNK - 1) // CHUNK
    return planes * (4 * N + 16 * chunks + 4 * frames * (2 * spec.n_states + 4) + 2 * frames * spec.n_states) + 64


def _launch(ctx, spec, stage, stream, B, C, frames, n, **kw):
    a = dict(d_src=None, stride=0, d_valid=None, d_nccf=None, d_raw=None, d_out=None)
    a.update(kw)
    t = spec.tables()
    ctx().kaldi_pitch_device(a["d_src"], B, C, a["stride"], frames, a["d_valid"], spec.sample_rate, spec.resample_freq, spec.win_length,
                             spec.hop_length, spec.window, spec.shift, spec.first_lag, spec.last_lag, spec.n_states, spec.phases,
                             spec.in_per_unit, t["down"].shape[1], t["up"].shape[1], spec.flags, spec.normalization_left_context,
                             spec.normalization_right_context, spec.delta_window, a["d_table"], a["d_nccf"], a["d_raw"], a["d_out"], n,
                             stage=stage, stream=stream)


def _checked(pcm, spec, lengths):
    import torch

    _spec_ok(spec)
    stride = _planes("pcm", pcm)
    B, C, T = pcm.shape
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        _lengths_host("lengths", lengths, B, T)
    n = int(spec.frames(T))
    if _scratch_bytes(spec, B * C, T, n) > SCRATCH_MAX:
        raise ValueError(f"{B * C} lines of {n} frames and {spec.n_states} states: the NCCF planes and backpointers would pass 2^31 bytes")
    return stride, B, C, T, n, _lengths_device("lengths", lengths, B, pcm.device)


def _kaldi_pitch(ctx, pcm, spec, lengths, out):
    """`kaldi_pitch` behind its first check, on pcm [B, C, T]; ctx() gives the context that runs it (the corpus's own inside
    `Corpus.crops`); out: a contiguous float32 tensor [B, C, lines, T'] to write, or None for a new one"""
    import torch

    stride, B, C, T, n, d_valid = _checked(pcm, spec, lengths)
    shape = (B, C, spec.lines, n)
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
    with torch.cuda.device(pcm.device):
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _launch(ctx, spec, 0, stream, B, C, T, n, d_src=pcm, stride=stride, d_valid=d_valid, d_table=_table_device(spec, pcm.device), d_out=out)
    return out


def kaldi_pitch(pcm, spec, lengths=None, out=None):
    """Kaldi's pitch features on the GPU: pcm float32 [B, C, T] on the device, contiguous or the slice [..., :T] of a contiguous
    tensor (what lies behind the slice is not read); spec: a `KaldiPitch`; lengths: [B] integers, a sequence or a tensor (-1
    counts as 0, more than T as T); default: T.  Returns float32 [B, C, lines, T'], T' = spec.frames(T): with process=False
    the POV NCCF at the decoded lag and the pitch in Hz (compute-kaldi-pitch-feats' output transposed), with process=True the
    selected processed lines in Kaldi's order; zeros at and behind a row's frame count (see the module).  out: a contiguous
    tensor of that shape apart from pcm; default: a new one.  Three launches, asynchronous on the current stream, nothing is
    read back; ValueError where the context's scratch would pass 2^31 bytes, and for every other bad argument, before any
    device work."""
    ctx = _device_context("pcm", pcm, "[B, C, T]")
    return _kaldi_pitch(ctx, pcm, spec, lengths, out)


def kaldi_pitch_nccf(pcm, spec, lengths=None):
    """The downsampler and the NCCF alone: pcm and lengths as for `kaldi_pitch` to float32 [B, C, 2, T', n_states], the pitch
    NCCF (with the ballast) and the POV NCCF (without) on the lag grid; zeros at and behind a row's frame count"""
    import torch

    ctx = _device_context("pcm", pcm, "[B, C, T]")
    stride, B, C, T, n, d_valid = _checked(pcm, spec, lengths)
    nccf = torch.zeros((B, C, 2, n, spec.n_states), dtype=torch.float32, device=pcm.device)
    if nccf.numel() == 0:
        return nccf
    with torch.cuda.device(pcm.device):
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _launch(ctx, spec, 1, stream, B, C, T, n, d_src=pcm, stride=stride, d_valid=d_valid, d_table=_table_device(spec, pcm.device), d_nccf=nccf)
    return nccf


def _lines_device(t, name, spec, inner, frame_counts):
    import torch

    _spec_ok(spec)
    want = f"a contiguous float32 device tensor [B, C, {', '.join(str(i) for i in inner)}]"
    if (t.dtype != torch.float32 or t.dim() != 2 + len(inner) or t.shape[1] == 0 or not t.is_contiguous()
            or tuple(t.shape[2:3] + t.shape[4:]) != tuple(inner[:1] + inner[2:])):
        raise ValueError(f"{name} must be {want}")
    B, n = t.shape[0], t.shape[3]
    if frame_counts is not None and not isinstance(frame_counts, torch.Tensor):
        _lengths_host("frame_counts", frame_counts, B, n)
    return B, t.shape[1], n, _lengths_device("frame_counts", frame_counts, B, t.device)


def kaldi_pitch_decode(nccf, spec, frame_counts=None):
    """The decode alone, on given NCCFs: nccf a contiguous float32 device tensor [B, C, 2, T', n_states] of finite values;
    frame_counts: [B] integers, a sequence or a tensor (below 0 counts as 0, more than T' as T'); default: T'.  Returns the
    raw track float32 [B, C, 2, T'] (`kaldi_pitch_decode_host` with f32=True, bit for bit)."""
    import torch

    ctx = _device_context("nccf", nccf, "[B, C, 2, T', n_states]")
    B, C, n, d_counts = _lines_device(nccf, "nccf", spec, (2, "T'", spec.n_states), frame_counts)
    if 2 * B * C * n * spec.n_states + 64 > SCRATCH_MAX:
        raise ValueError(f"{B * C} lines of {n} frames and {spec.n_states} states: the backpointers would pass 2^31 bytes")
    raw = torch.zeros((B, C, 2, n), dtype=torch.float32, device=nccf.device)
    if raw.numel() == 0:
        return raw
    with torch.cuda.device(nccf.device):
        stream = torch.cuda.current_stream(nccf.device).cuda_stream
        _launch(ctx, spec, 2, stream, B, C, n, n, d_valid=d_counts, d_table=_table_device(spec, nccf.device), d_nccf=nccf, d_raw=raw)
    return raw


def kaldi_pitch_process(raw, spec, frame_counts=None):
    """The post-processing alone, on a given raw track: raw a contiguous float32 device tensor [B, C, 2, T'] (the POV NCCF and
    the pitch in Hz, above 0 inside a row's count); frame_counts as for `kaldi_pitch_decode`.  Returns float32
    [B, C, lines, T'] (`kaldi_pitch_process_host` with f32=True, bit for bit).  ValueError for a spec with process=False."""
    import torch

    ctx = _device_context("raw", raw, "[B, C, 2, T']")
    B, C, n, d_counts = _lines_device(raw, "raw", spec, (2, "T'"), frame_counts)
    if not spec.process:
        raise ValueError("spec.process is False: there is nothing to post-process")
    out = torch.zeros((B, C, spec.lines, n), dtype=torch.float32, device=raw.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(raw.device):
        stream = torch.cuda.current_stream(raw.device).cuda_stream
        _launch(ctx, spec, 3, stream, B, C, n, n, d_valid=d_counts, d_table=_table_device(spec, raw.device), d_raw=raw, d_out=out)
    return out
