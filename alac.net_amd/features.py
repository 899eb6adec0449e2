"""Log-mel features behind the decode: framing, window, DFT, power, mel projection and log in one kernel
(alacgpu_logmel_device, csrc/alac_features.hip).

A row is x[0 .. L) float32 with L > n_fft // 2; n_bins = n_fft // 2 + 1.  Frame t of 0 .. T', T' = 1 + L // hop, is centred on
sample t * hop:

    x_t[n]    = x[t * hop - n_fft // 2 + n],  n < n_fft, reflected at both ends: index -i reads x[i], index L - 1 + i reads
                x[L - 1 - i] (torch.stft's center=True, pad_mode="reflect")
    X[j]      = sum over n of (window[n] * x_t[n]) * basis[n, j],   j < 2 * n_bins
    P[k]      = X[k]^2 + X[n_bins + k]^2
    M[m]      = sum over k of fb[m, k] * P[k]
    out[m, t] = log(max(M[m], floor))        (or M[m] itself with log=None)

    window[n]            = 0.5 - 0.5 cos(2 pi n / n_fft)                       the periodic Hann window
    basis[n, k]          = cos(2 pi ((n k) mod n_fft) / n_fft)
    basis[n, n_bins + k] = -sin(2 pi ((n k) mod n_fft) / n_fft)                the angle reduced in integers first
    fb                   = mel_filterbank(...), or the caller's

Each table is built in float64 and rounded to float32 once.  One reflection brings every index inside 0 .. L except, with an
odd n_fft and L = n_fft // 2 + 1, the last tap of a last frame centred on L: that tap counts as zero.  What lies behind a
crop's length is the zeros `crops` wrote: the transform sees the padded row, as a dataloader would.

The kernel evaluates this in float32: one rounding of window[n] * x_t[n], then fused multiply-adds in ascending n and k.  With
u = 2^-24 and a_n = |window[n] * x_t[n]| that stays within

    delta_j = (n_fft + 2) u sum over n of a_n |basis[n, j]|
    dP_k    = 2 |Re| delta_re + delta_re^2 + 2 |Im| delta_im + delta_im^2 + 3 u P_k
    dM_m    = sum over k of fb[m, k] dP_k + (n_bins + 1) u M_m            (|fb| for a filterbank with negative weights)

of the exact value; `logmel_host(..., bound=True)` returns dM.

Input that is not finite follows IEEE arithmetic and is never hidden.  A NaN or an infinity at sample i reaches the frames that
have a tap on i -- the tap whose window weight is zero too, 0 * inf being NaN -- and only those: every other frame, and every
other plane, is bit for bit what it is for the same signal without it.  In such a frame an element is whatever the sums above
give in IEEE arithmetic (with the tables of this module NaN throughout: every filter has a weight of zero somewhere, and
0 * inf is NaN), and max(M, floor) keeps a NaN as np.maximum and torch.clamp do: its log is NaN, never log(floor).  Where the
sums do give +inf the log is +inf.

`mel_filterbank`, `LogMel` and `logmel_host` (the kernel's specification in numpy) need no device.  `log_mel` is the call on
device tensors.
"""
import math

import numpy as np

MIN_NFFT, MAX_NFFT, MAX_MELS = 16, 2048, 256
_LOGS = {None: 0, "ln": 1, "log10": 2}
_U = 2.0 ** -24

# the Slaney scale: linear below 1000 Hz, logarithmic above
_SLANEY_BREAK_HZ = 1000.0
_SLANEY_BREAK_MEL = 15.0                                       # 1000 / (200 / 3)
_SLANEY_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f, scale="slaney"):
    """Hz to mel (float64 arrays too).  slaney: f / (200 / 3) below 1000 Hz, 15 + ln(f / 1000) / (ln(6.4) / 27) above;
    htk: 2595 log10(1 + f / 700)."""
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    if scale != "slaney":
        raise ValueError(f"scale must be 'slaney' or 'htk', not {scale!r}")
    return np.where(f < _SLANEY_BREAK_HZ, f * 3.0 / 200.0,
                    _SLANEY_BREAK_MEL + np.log(np.maximum(f, _SLANEY_BREAK_HZ) / _SLANEY_BREAK_HZ) / _SLANEY_LOGSTEP)


def mel_to_hz(m, scale="slaney"):
    """The inverse of `hz_to_mel`."""
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if scale != "slaney":
        raise ValueError(f"scale must be 'slaney' or 'htk', not {scale!r}")
    return np.where(m < _SLANEY_BREAK_MEL, m * 200.0 / 3.0,
                    _SLANEY_BREAK_HZ * np.exp(_SLANEY_LOGSTEP * (np.maximum(m, _SLANEY_BREAK_MEL) - _SLANEY_BREAK_MEL)))


def _int(name, v, lo, hi=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{name} must be an integer of {lo} .. {hi if hi is not None else ''}, not {v!r}")
    return int(v)


def _band(sample_rate, f_min, f_max):
    f_min = float(f_min)
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    if not (0.0 <= f_min < f_max <= sample_rate / 2.0):
        raise ValueError(f"0 <= f_min < f_max <= sample_rate / 2 does not hold for f_min = {f_min}, f_max = {f_max}, "
                         f"sample_rate = {sample_rate}")
    return f_min, f_max


def mel_filterbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None, scale="slaney", norm="slaney"):
    """The mel filterbank, float32 [n_mels, n_fft // 2 + 1], computed in float64 and rounded once: triangular filters over
    n_mels + 2 points f_0 .. f_{n_mels + 1} equally spaced on the mel scale between f_min and f_max (default sample_rate / 2);
    filter m rises from f_m to 1 at f_{m + 1} and falls to 0 at f_{m + 2}, evaluated at the bin frequencies
    k * sample_rate / n_fft.  norm="slaney" scales filter m by 2 / (f_{m + 2} - f_m) (unit area in Hz); norm=None leaves the
    peaks at 1.  ValueError: limits as `LogMel`'s, an unknown scale or norm."""
    sample_rate = _int("sample_rate", sample_rate, 1)
    n_fft = _int("n_fft", n_fft, MIN_NFFT, MAX_NFFT)
    n_mels = _int("n_mels", n_mels, 1, MAX_MELS)
    f_min, f_max = _band(sample_rate, f_min, f_max)
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be 'slaney' or None, not {norm!r}")
    pts = mel_to_hz(np.linspace(hz_to_mel(f_min, scale), hz_to_mel(f_max, scale), n_mels + 2), scale)      # [n_mels + 2]
    bins = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / n_fft)
    rise = (bins[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    fall = (pts[2:, None] - bins[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(rise, fall))
    if norm == "slaney":
        fb = fb * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return fb.astype(np.float32)


def hann_window(n_fft):
    """0.5 - 0.5 cos(2 pi n / n_fft), float32 [n_fft]"""
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(np.float32)


def dft_basis(n_fft, rows=None):
    """float32 [rows, 2 * n_bins], rows = n_fft unless given (fbank's window is shorter than its n_fft: the zeros that pad a
    frame have no rows): cos and -sin of 2 pi ((n k) mod n_fft) / n_fft"""
    n_bins = n_fft // 2 + 1
    rows = n_fft if rows is None else rows
    nk = (np.arange(rows, dtype=np.int64)[:, None] * np.arange(n_bins, dtype=np.int64)[None, :]) % n_fft
    ang = 2.0 * np.pi * (nk.astype(np.float64) / n_fft)
    return np.concatenate([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)


class _Transform:
    """What `LogMel`, `fbank.KaldiFbank` and `mfcc.KaldiMfcc` share: read-only float32 tables (window, basis, fb; a subclass
    names more in `_TABLES`) beside their own fields, immutability, and the tables on a device.  What `Corpus.crops` and
    `_on_device` need of a transform is the subclass's: `frames`, `min_frames`, `short`, `lengths` and `launch`."""

    __slots__ = ("window", "basis", "fb", "_device")
    _TABLES = ("window", "basis", "fb")

    def _freeze(self, window, basis, fb, **fields):
        """The end of a subclass's __init__: the tables made read-only, and they and the fields assigned"""
        fields = dict(fields, window=window, basis=basis, fb=fb, _device={})
        for name in self._TABLES:
            fields[name].flags.writeable = False
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError(f"a {type(self).__name__} is immutable")

    def __delattr__(self, name):
        raise AttributeError(f"a {type(self).__name__} is immutable")

    def device_tables(self, device):
        """The tables (window, basis, fb and what else `_TABLES` names) on the device (a torch.device), uploaded once per device"""
        import torch

        index = device.index if device.index is not None else torch.cuda.current_device()
        if index not in self._device:
            dev = torch.device("cuda", index)
            self._device[index] = tuple(torch.from_numpy(np.array(getattr(self, a))).to(dev) for a in self._TABLES)
        return self._device[index]


class LogMel(_Transform):
    """An immutable description of a log-mel transform together with its three float32 tables: `window` [n_fft], `basis`
    [n_fft, 2 * n_bins] and `fb` [n_mels, n_bins] (read-only arrays).  filterbank: the caller's own [n_mels, n_bins] array
    instead of `mel_filterbank` (n_mels is then its row count; f_min, f_max, scale and norm describe nothing).  log: "ln",
    "log10", or None for mel power (floor is then ignored).  ValueError unless 16 <= n_fft <= 2048, 1 <= hop_length <= n_fft,
    1 <= n_mels <= 256, floor > 0 and finite, 0 <= f_min < f_max <= sample_rate / 2."""

    __slots__ = ("sample_rate", "n_fft", "hop_length", "n_mels", "n_bins", "f_min", "f_max", "scale", "norm", "log", "floor")

    def __init__(self, sample_rate, n_fft=400, hop_length=160, n_mels=80, f_min=0.0, f_max=None, scale="slaney", norm="slaney",
                 log="ln", floor=1e-10, filterbank=None):
        sample_rate = _int("sample_rate", sample_rate, 1)
        n_fft = _int("n_fft", n_fft, MIN_NFFT, MAX_NFFT)
        hop_length = _int("hop_length", hop_length, 1, n_fft)
        n_bins = n_fft // 2 + 1
        if log not in _LOGS:
            raise ValueError(f"log must be 'ln', 'log10' or None, not {log!r}")
        floor = float(floor)
        if not (floor > 0.0 and math.isfinite(floor) and math.isfinite(float(np.float32(floor))) and float(np.float32(floor)) > 0.0):
            raise ValueError(f"floor must be positive and finite in float32, not {floor!r}")
        f_min, f_max = _band(sample_rate, f_min, f_max)
        if filterbank is None:
            n_mels = _int("n_mels", n_mels, 1, MAX_MELS)
            fb = mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max, scale, norm)
        else:
            fb = np.array(filterbank, dtype=np.float32, order="C")
            if fb.ndim != 2 or fb.shape[1] != n_bins or not 1 <= fb.shape[0] <= MAX_MELS:
                raise ValueError(f"filterbank must be [1 .. {MAX_MELS}, {n_bins}], not {fb.shape}")
            n_mels = fb.shape[0]
        self._freeze(hann_window(n_fft), dft_basis(n_fft), fb, sample_rate=sample_rate, n_fft=n_fft, hop_length=hop_length,
                     n_mels=n_mels, n_bins=n_bins, f_min=f_min, f_max=f_max, scale=scale, norm=norm, log=log, floor=floor)

    def __repr__(self):
        return (f"LogMel(sample_rate={self.sample_rate}, n_fft={self.n_fft}, hop_length={self.hop_length}, n_mels={self.n_mels}, "
                f"log={self.log!r}, floor={self.floor})")

    @property
    def log_mode(self):
        """alacgpu_logmel_device's log_mode: 0 none, 1 ln, 2 log10"""
        return _LOGS[self.log]

    def frames(self, L):
        """T' = 1 + L // hop_length (numpy arrays too)"""
        return 1 + L // self.hop_length

    # what `Corpus.crops` needs of a transform (fbank.KaldiFbank has the same four): the shortest row, what refuses a shorter
    # one, the device lengths and the launch
    @property
    def min_frames(self):
        """The shortest row the transform takes: n_fft // 2 + 1"""
        return self.n_fft // 2 + 1

    def short(self, L):
        """What refuses a row of L < min_frames samples"""
        return f"num_frames {L}: the transform needs more than n_fft // 2 = {self.n_fft // 2}"

    def lengths(self, lengths):
        """`feature_lengths(lengths, hop_length)`"""
        return feature_lengths(lengths, self.hop_length)

    def launch(self, gpu, src, rows, channels, src_stride, L, out, stream):
        """The features of src (float32 device tensor, planar [rows, channels, src_stride], the first L of a plane are signal)
        into out [rows, channels, n_mels, frames(L)] by the AlacGpuContext `gpu`: one alacgpu_logmel_device call on `stream`"""
        window, basis, fb = self.device_tables(src.device)
        gpu.logmel_device(src, rows, channels, src_stride, L, self.n_fft, self.hop_length, self.n_mels, window, basis, fb,
                          self.log_mode, self.floor, out, self.frames(L), stream=stream)


def frame_index(L, n_fft, hop):
    """(idx int64 [T', n_fft], inside bool [T', n_fft]): where frame t's tap n reads x, after the reflection; `inside` is False
    for a tap that one reflection does not bring into 0 .. L (it counts as zero; idx is 0 there)."""
    T = 1 + L // hop
    g = np.arange(T, dtype=np.int64)[:, None] * hop - n_fft // 2 + np.arange(n_fft, dtype=np.int64)[None, :]
    g = np.where(g < 0, -g, np.where(g >= L, 2 * (L - 1) - g, g))
    inside = (g >= 0) & (g < L)
    return np.where(inside, g, 0), inside


def logmel_host(x, spec, bound=False):
    """The kernel's specification in numpy: x float32 [..., L], L > n_fft // 2, to float64 [..., n_mels, T'] -- float64
    arithmetic on the float32 input and the float32 tables of `spec`.  bound=True: returns (out, dM), dM float64 like out:
    how far a float32 evaluation with one rounding per window product and fused multiply-add chains may be from M (the
    module docstring's bound; in the power domain whatever spec.log is)."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    L = x.shape[-1] if x.ndim else 0
    if x.ndim < 1 or L <= spec.n_fft // 2:
        raise ValueError(f"x must be [..., L] with L > n_fft // 2 = {spec.n_fft // 2}, not {x.shape}")
    n_bins = spec.n_bins
    idx, inside = frame_index(L, spec.n_fft, spec.hop_length)
    T = idx.shape[0]
    w = spec.window.astype(np.float64)
    basis = spec.basis.astype(np.float64)
    fb = spec.fb.astype(np.float64)
    rows = x.reshape(-1, L).astype(np.float64)
    out = np.empty((rows.shape[0], spec.n_mels, T), dtype=np.float64)
    dM = np.empty_like(out) if bound else None
    for r, row in enumerate(rows):
        fr = np.where(inside, row[idx], 0.0) * w[None, :]           # [T, n_fft]
        X = fr @ basis                                               # [T, 2 n_bins]
        P = X[:, :n_bins] ** 2 + X[:, n_bins:] ** 2
        M = P @ fb.T                                                 # [T, n_mels]
        if bound:
            d = (spec.n_fft + 2) * _U * (np.abs(fr) @ np.abs(basis))
            dre, dim = d[:, :n_bins], d[:, n_bins:]
            dP = 2 * np.abs(X[:, :n_bins]) * dre + dre ** 2 + 2 * np.abs(X[:, n_bins:]) * dim + dim ** 2 + 3 * _U * P
            dM[r] = (dP @ np.abs(fb).T + (n_bins + 1) * _U * (P @ np.abs(fb).T)).T
        if spec.log is not None:
            M = np.maximum(M, float(np.float32(spec.floor)))
            M = np.log(M) if spec.log == "ln" else np.log10(M)
        out[r] = M.T
    out = out.reshape(x.shape[:-1] + (spec.n_mels, T))
    return (out, dM.reshape(out.shape)) if bound else out


def _chain(a, b):
    """a [T, K] float32, b [K, N] float64 holding float32 values: fma(a[:, k], b[k], acc) for k = 0 .. K - 1, from zero (an
    fma of float32 values as the exact float64 product plus the float64 addend, rounded to float64 and then to float32: twice
    where the hardware rounds once, which differs in the last bit of rare elements only)"""
    a = np.ascontiguousarray(a.T, dtype=np.float64)                 # [K, T]
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    wide = np.zeros(acc.shape, dtype=np.float64)
    tmp = np.empty_like(wide)
    for k in range(a.shape[0]):
        np.multiply(a[k][:, None], b[k][None, :], out=tmp)
        tmp += wide
        acc[...] = tmp                                               # the rounding to float32
        wide[...] = acc
    return acc


def logmel_host_f32(x, spec):
    """The kernel's arithmetic in numpy, one float32 operation at a time: x float32 [..., L] to float32 [..., n_mels, T'], the
    mel power (spec.log and spec.floor are not applied).  The window product is rounded once; X[j] is a chain of fused
    multiply-adds in ascending n from zero; P = fma(re, re, round(im * im)); M[m] is a chain of fused multiply-adds in
    ascending k from zero.  (An fma of float32 values is evaluated as the float64 product, which is exact, plus the float64
    addend, rounded to float64 and then to float32: twice where the hardware rounds once, which differs in the last bit of
    rare elements only.)  Its distance from `logmel_host` is what a correct float32 evaluation costs: the tests hold the
    kernel to a small multiple of that, far inside dM."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    L = x.shape[-1] if x.ndim else 0
    if x.ndim < 1 or L <= spec.n_fft // 2:
        raise ValueError(f"x must be [..., L] with L > n_fft // 2 = {spec.n_fft // 2}, not {x.shape}")
    f32, f64 = np.float32, np.float64
    n_bins = spec.n_bins
    idx, inside = frame_index(L, spec.n_fft, spec.hop_length)
    T = idx.shape[0]
    basis = spec.basis.astype(f64)
    fb = spec.fb.astype(f64)
    rows = x.reshape(-1, L)
    out = np.empty((rows.shape[0], spec.n_mels, T), dtype=f32)

    for r, row in enumerate(rows):
        fr = (np.where(inside, row[idx], f32(0)) * spec.window[None, :]).astype(f32)       # [T, n_fft]
        X = _chain(fr, basis)
        re, im = X[:, :n_bins].astype(f64), X[:, n_bins:].astype(f64)
        P = (re * re + (im * im).astype(f32).astype(f64)).astype(f32)
        out[r] = _chain(P, np.ascontiguousarray(fb.T)).T
    return out.reshape(x.shape[:-1] + (spec.n_mels, T))


# ---- on the device -------------------------------------------------------------------------------------------------------------
def feature_lengths(lengths, hop):
    """lengths // hop + 1 where lengths >= 0, -1 where it is -1 (an int64 tensor)"""
    import torch

    return torch.where(lengths >= 0, torch.div(lengths, hop, rounding_mode="floor") + 1, torch.full_like(lengths, -1))


def _on_device(pcm, spec, kind, takes, short, lengths):
    """`log_mel`, `fbank.fbank` and `mfcc.mfcc` behind their names: spec is a `kind`, pcm a float32 device tensor whose shape the messages
    call `takes` and for whose T `short(T)` is None (the ValueError's text otherwise); the output, one `spec.launch` over all
    planes unless there is nothing to compute, and `spec.lengths` of the lengths"""
    import torch

    from ._stageargs import _device_context

    if not isinstance(spec, kind):
        raise ValueError(f"spec must be a {kind.__name__}")
    ctx = _device_context("pcm", pcm, "[..., T]")
    if pcm.dtype != torch.float32 or pcm.dim() < 1:
        raise ValueError(f"pcm must be a float32 device tensor {takes}")
    T = pcm.shape[-1]
    if short(T) is not None:
        raise ValueError(short(T))
    dev = pcm.device
    planes = int(np.prod(pcm.shape[:-1], dtype=np.int64))
    Tf = spec.frames(T)
    out = torch.empty(tuple(pcm.shape[:-1]) + (spec.n_mels, Tf), dtype=torch.float32, device=dev)
    if planes and Tf:
        with torch.cuda.device(dev):
            spec.launch(ctx(), pcm.contiguous(), planes, 1, T, T, out, torch.cuda.current_stream(dev).cuda_stream)
    if lengths is None:
        return out
    lens = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths, dtype=np.int64))
    if lens.dtype.is_floating_point:
        raise ValueError("lengths must be integers")
    return out, spec.lengths(lens.to(torch.int64))


def log_mel(pcm, spec, lengths=None):
    """Log-mel features on the GPU: pcm float32 [..., T] on the device (as `load`, `load_batch` and `crops` return it),
    T > n_fft // 2, to float32 [..., spec.n_mels, 1 + T // hop]; one kernel, asynchronous on the current stream.  Every row is
    transformed over its whole T (what lies behind a file's or a crop's length is the zeros the decode wrote).  lengths
    (a sequence or an integer tensor): returns (features, lengths // hop + 1 as an int64 tensor where `lengths` was; an
    entry of -1 stays -1)."""
    def short(T):
        if T <= spec.n_fft // 2:
            return f"T = {T} frames: the transform needs more than n_fft // 2 = {spec.n_fft // 2}"

    return _on_device(pcm, spec, LogMel, "[..., T]", short, lengths)
