"""The stage keywords of a crop step -- `speed`, `pitch`, `mix`, `reverb`, `level`, `effects`, `f0`, `features`, `deltas`, `vad`,
`normalize`, `augment`, and `sample_rate` / `mono` -- in front of any device work, for the two callers `Corpus.crops` and
`Corpus.random_crops`.  `_stage_plan` is the one check: it takes the facts of a call as plain values and the keywords, refuses
what a stage cannot take (in the order of its `_StagePlan` fields) and returns the record every later step reads;
`_for_batch` adds the refusals that need the batch size; `_middle_draws` fills the draws that were not given, from a generator
or from the device's default one.  A new stage gets a field of `_StagePlan`, its refusals in a `_*_given` here, its draws in
`_middle_draws` if it has any, and its run in `Corpus._run`.
"""
import collections

from . import _frame_count, _torch_dtype
from .augment import LDS_MAX as _WARP_MAX, _check_draws, _how
from .biquad import Effects
from .cqt import ConstantQ
from .deltas import Deltas
from .fbank import KaldiFbank
from .kaldi_pitch import KaldiPitch
from .features import LogMel
from .level import _checked as _level_checked
from .mfcc import KaldiMfcc
from .mix import AddNoise
from .normalize import MeanVar, TopDb
from .pcen import Pcen
from .pitch import PitchShift
from .pyin import PYin
from .reverb import Reverb
from .sliding import LDS_MAX as _SLIDING_LDS_MAX, RING_WINDOW_MAX as _SLIDING_RING_WINDOW_MAX, SlidingMeanVar
from .speed import SpeedPerturb
from .stft import Spectrogram
from .vad import EnergyVad
from .yin import Yin

_NEEDS_RATE = "the files of this corpus differ in sample rate: crops need sample_rate="
_TWO_CHANNELS = "{n} channels: the resampler takes 1 or 2"
_FEATURES = (LogMel, KaldiFbank, KaldiMfcc, ConstantQ, Spectrogram)              # what crops(features=) takes
# The drawing stages for `_pair`: the keyword, the specification's class and the messages' nouns; for `_second_corpus` also the
# attribute that holds the second corpus, how many tensors its draw() returns and what their dtypes have to be
_MIX = dict(arg="mix", spec=AddNoise, corpus="noise", theirs="the noise corpus", they="the noise",
            what="mix must be a mix.AddNoise or (AddNoise, what its draw() returned)",
            draws=3, dtypes=lambda torch, files, offsets, snr_db: snr_db.is_floating_point,
            tensors="the three tensors (noise_files, noise_offsets, snr_db) of AddNoise.draw", f32="noise is mixed into float32 crops",
            channels="a noise corpus of {n} channels into crops of {Co}: it can become one channel from 1 or 2 only")
_SPEED = dict(arg="speed", spec=SpeedPerturb, what="speed must be a speed.SpeedPerturb or (SpeedPerturb, what its draw() returned)",
              f32="float32 crops are speed-perturbed")
_PITCH = dict(arg="pitch", spec=PitchShift, what="pitch must be a pitch.PitchShift or (PitchShift, what its draw() returned)",
              f32="float32 crops are pitch-shifted")
_REVERB = dict(arg="reverb", spec=Reverb, corpus="rirs", theirs="the corpus of impulse responses", they="the responses",
               what="reverb must be a reverb.Reverb or (Reverb, what its draw() returned)",
               draws=2, dtypes=lambda torch, files, keep: not files.is_floating_point and keep == torch.bool,
               tensors="the two tensors (rir_files, keep) of Reverb.draw", f32="float32 crops are reverberated",
               channels="impulse responses of {n} channels into crops of {Co}: they can become one channel from 1 or 2 only")
_EFFECTS = dict(arg="effects", spec=Effects, what="effects must be a biquad.Effects or (Effects, what its draw() returned)",
                f32="float32 crops are filtered")

# What `_stage_plan` returns (its docstring states the fields): a field per keyword, and what every later step derives from them
_StagePlan = collections.namedtuple("_StagePlan", "speed pitch mix reverb level effects f0 features deltas vad normalize augment "
                                                  "sample_rate mono rate Co L lines frames")


def _is_f32(torch, dtype):
    return _torch_dtype(torch, torch.float32 if dtype is None else dtype) == torch.float32


def _float32(torch, dtype, message):
    if not _is_f32(torch, dtype):
        raise ValueError(message)


def _has_rate(rate, also=""):
    if rate is None:
        raise ValueError(_NEEDS_RATE + also)


def _pair(given, stage):
    """A drawing stage's keyword as the pair (its specification, draws or None); ValueError for anything else"""
    spec, draws = given if isinstance(given, tuple) and len(given) == 2 else (given, None)
    if not isinstance(spec, stage["spec"]):
        raise ValueError(f"{stage['what']}, not {given!r}")
    return spec, draws


def _index_draws(torch, draws, stage, device):
    """The draws of speed= and pitch=: None or an integer tensor [B] on the device; B is `_for_batch`'s to check"""
    if draws is not None and (not isinstance(draws, torch.Tensor) or draws.dim() != 1 or draws.dtype.is_floating_point
                              or draws.dtype == torch.bool or draws.device != device):
        raise ValueError(f"the draws of {stage['arg']}= must be the integer tensor [B] of {stage['spec'].__name__}.draw on {device}")


def _on_device(draws, stage, device):
    if any(t.device != device for t in draws):
        raise ValueError(f"the draws of {stage['arg']}= must be on {device}")


def _speed_given(torch, given, channels, dtype, rate, device):
    """crops(speed=) as the pair (SpeedPerturb, draws or None): ValueError for anything else, for int32 crops, for a corpus of
    more than 2 channels and for crops without a rate"""
    spec, draws = _pair(given, _SPEED)
    _float32(torch, dtype, _SPEED["f32"])
    if channels not in (1, 2):
        raise ValueError(_TWO_CHANNELS.format(n=channels))
    _has_rate(rate)
    _index_draws(torch, draws, _SPEED, device)
    return spec, draws


def _pitch_given(torch, given, dtype, rate, Co, num_frames, device):
    """crops(pitch=) as the pair (PitchShift, draws or None): ValueError for anything else, for int32 crops, for crops of more
    than 2 channels or without a rate and for crops too short to reflect"""
    spec, draws = _pair(given, _PITCH)
    _float32(torch, dtype, _PITCH["f32"])
    if Co not in (1, 2):
        raise ValueError(f"{Co} channels: the resampler behind the vocoder takes 1 or 2")
    _has_rate(rate)
    L = _frame_count("num_frames", num_frames)
    if L <= spec.n_fft // 2:
        raise ValueError(f"crops of {L} frames: a PitchShift of n_fft {spec.n_fft} reflects {spec.n_fft // 2} and needs more")
    _index_draws(torch, draws, _PITCH, device)
    return spec, draws


def _second_corpus(torch, given, stage, dtype, rate, Co, device):
    """crops(mix=) or crops(reverb=) (`stage`: _MIX or _REVERB) as the pair (its specification, draws or None): ValueError for
    anything else, for int32 crops, for a second corpus that is closed, on another device or of a channel count that crops of
    Co channels cannot take, and for crops without a rate.  Of the second corpus it asks `_gpu`, `_dev` and `channels` only."""
    spec, draws = _pair(given, stage)
    if stage is _REVERB and spec.rooms is not None:
        return _rooms_given(torch, spec, draws, dtype, rate, device)
    if draws is not None:
        ok = isinstance(draws, tuple) and len(draws) == stage["draws"] and all(isinstance(t, torch.Tensor) and t.dim() == 1
                                                                               for t in draws)
        if not ok or any(t.shape != draws[0].shape for t in draws) or not stage["dtypes"](torch, *(t.dtype for t in draws)):
            raise ValueError(f"the draws of {stage['arg']}= must be {stage['tensors']}")
        _on_device(draws, stage, device)
    _float32(torch, dtype, stage["f32"])
    other = getattr(spec, stage["corpus"])
    if other._gpu is None:
        raise ValueError(f"{stage['theirs']} is closed")
    if other._dev != device:
        raise ValueError(f"{stage['theirs']} is on {other._dev}, the crops on {device}")
    _has_rate(rate, f", and {stage['they']} a rate to crop at")
    if other.channels != Co and other.channels not in (1, 2):
        raise ValueError(stage["channels"].format(n=other.channels, Co=Co))
    return spec, draws


def _rooms_given(torch, spec, draws, dtype, rate, device):
    """`_second_corpus` for a Reverb over simulated rooms: the draws are (geometry float64 [B, 9], beta float32 [B, 6], keep
    bool [B]) on the device; ValueError for anything else, for int32 crops, for crops without a rate and for a policy whose
    smallest room is refused at that rate"""
    if draws is not None:
        ok = isinstance(draws, tuple) and len(draws) == 3 and all(isinstance(t, torch.Tensor) for t in draws)
        if not (ok and draws[0].dim() == 2 and draws[0].shape[1] == 9 and draws[0].dtype == torch.float64
                and draws[1].shape == (draws[0].shape[0], 6) and draws[1].dtype == torch.float32
                and draws[2].shape == (draws[0].shape[0],) and draws[2].dtype == torch.bool):
            raise ValueError("the draws of reverb= must be the three tensors (geometry, beta, keep) of Reverb.draw")
        _on_device(draws, _REVERB, device)
    _float32(torch, dtype, _REVERB["f32"])
    _has_rate(rate, ", and the responses a rate to be computed at")
    spec.check_rate(int(rate))
    return spec, draws


def _effects_given(torch, given, dtype, rate, device):
    """crops(effects=) as the pair (Effects, draws or None): ValueError for anything else, for int32 crops, for crops without a
    rate, for a filter at or above their Nyquist frequency and for draws that are not (float64 [B, S, 5], float64 [B]) on the
    device; B is `_for_batch`'s to check"""
    spec, draws = _pair(given, _EFFECTS)
    _float32(torch, dtype, _EFFECTS["f32"])
    _has_rate(rate)
    spec.check_rate(rate)
    if draws is not None:
        ok = isinstance(draws, tuple) and len(draws) == 2 and all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 for t in draws)
        if not ok or draws[0].dim() != 3 or tuple(draws[0].shape[1:]) != (spec.sections, 5) or draws[1].shape != draws[0].shape[:1]:
            raise ValueError(f"the draws of effects= must be the two float64 tensors (coeffs [B, {spec.sections}, 5], gain [B]) of "
                             f"Effects.draw")
        _on_device(draws, _EFFECTS, device)
    return spec, draws


def _f0_given(torch, spec, dtype, rate, vad, num_frames):
    """crops(f0=): ValueError for what is neither a Yin nor a PYin nor a KaldiPitch, for one of another rate than the crops', for int32 crops,
    together with vad= and for crops too short for a frame"""
    if not isinstance(spec, (Yin, PYin, KaldiPitch)):
        raise ValueError(f"f0 must be a yin.Yin or a pyin.PYin, not {spec!r}; the third kind taken is a kaldi_pitch.KaldiPitch")
    _has_rate(rate)
    if spec.sample_rate != rate:
        raise ValueError(f"f0 for {spec.sample_rate} Hz, crops at {rate} Hz")
    _float32(torch, dtype, "F0 is estimated from float32 crops")
    if vad is not None:
        raise ValueError("f0= with vad=: the selected frames would no longer line up with the track")
    L = _frame_count("num_frames", num_frames)
    if L < spec.min_frames:
        raise ValueError(spec.short(L))


def _normalize_given(torch, normalize, features, deltas, dtype, num_frames):
    """crops(normalize=), in front of the check of features= (which may still be anything): ValueError for what is none of the
    four kinds, for a Pcen without energies to compress, a TopDb without features, int32 crops without features, and a
    SlidingMeanVar whose window the lines are too long for"""
    if not isinstance(normalize, (MeanVar, TopDb, SlidingMeanVar, Pcen)):
        raise ValueError(f"normalize must be a normalize.MeanVar, a normalize.TopDb, a sliding.SlidingMeanVar or a pcen.Pcen, "
                         f"not {normalize!r}")
    if isinstance(normalize, Pcen):
        if features is None:
            raise ValueError("a Pcen compresses mel or constant-Q energies: it needs features=")
        if isinstance(features, KaldiMfcc) or (isinstance(features, _FEATURES) and features.log not in (None, False)):
            raise ValueError(f"a Pcen compresses energies: features with log=None (a LogMel, a ConstantQ, a Spectrogram) or log=False "
                             f"(a KaldiFbank), not {features!r}")
        if deltas is not None:
            raise ValueError("a Pcen compresses energies: deltas= of them are none")
        if normalize.lines is not None and isinstance(features, _FEATURES) and normalize.lines != features.n_mels:
            raise ValueError(f"a Pcen with {normalize.lines} values per parameter, features with {features.n_mels} lines")
    if features is None and isinstance(normalize, TopDb):
        raise ValueError("a TopDb clamps log-mel features: it needs features=")
    if features is None and not _is_f32(torch, dtype):
        raise ValueError(f"a {type(normalize).__name__} normalises float32 crops")
    if isinstance(normalize, SlidingMeanVar) and normalize.window > _SLIDING_RING_WINDOW_MAX:
        n = _frame_count("num_frames", num_frames) if features is None else None
        if n is None and isinstance(features, _FEATURES):
            n = features.frames(_frame_count("num_frames", num_frames))
        if n is not None and n > _SLIDING_LDS_MAX:
            raise ValueError(f"lines of {n} frames: above {_SLIDING_LDS_MAX} a sliding window takes at most "
                             f"{_SLIDING_RING_WINDOW_MAX} frames")


def _features_given(torch, features, dtype, rate, later):
    """crops(features=): ValueError for what is none of `_FEATURES`, for crops without a rate or at another one, for int32 crops
    and for a complex spectrogram with one of the `later` stages (name -> what was given) behind it"""
    if not isinstance(features, _FEATURES):
        raise ValueError(f"features must be a features.LogMel or a fbank.KaldiFbank or a mfcc.KaldiMfcc or a cqt.ConstantQ or a stft.Spectrogram, not {features!r} "
                         f"(sample_rate= and mono= go by keyword)")
    _has_rate(rate)
    if features.sample_rate != rate:
        raise ValueError(f"features for {features.sample_rate} Hz, crops at {rate} Hz")
    _float32(torch, dtype, "features are computed from float32 crops")
    if isinstance(features, Spectrogram) and features.power is None:
        for name, given in later.items():
            if given is not None:
                raise ValueError(f"a Spectrogram with power=None gives real and imaginary parts: {name}= takes magnitudes, powers or their logs")


def _stage_plan(channels, own_rate, device, dtype, num_frames, sample_rate=None, mono=False, speed=None, pitch=None, mix=None,
                reverb=None, level=None, effects=None, f0=None, features=None, deltas=None, vad=None, normalize=None, augment=None):
    """Every refusal of a crop step that needs neither the device nor the batch size, in the order speed, pitch, mix, reverb,
    level, effects, f0, normalize, features, deltas, vad, augment: ValueError, or the `_StagePlan` of the call.  The facts of the
    call: the corpus's channel count, its own rate (None where its files differ), its device, and dtype, num_frames,
    sample_rate and mono as `Corpus.crops` was given them.  The waveform's own refusals are `Corpus._waveform`'s.
    The plan has a field per keyword -- (specification, draws or None) for speed, pitch, mix, reverb, effects and augment,
    the specification for the others, None for a stage that was not asked for -- and what the later steps derive from them:
    the rate and the channels of the crops, L (num_frames; None without a stage that needs it in front of the waveform),
    and with features= their lines behind the deltas and their frames."""
    import torch

    rate = own_rate if sample_rate is None else sample_rate
    Co = 1 if mono else channels
    if speed is not None:
        speed = _speed_given(torch, speed, channels, dtype, rate, device)
    if pitch is not None:
        pitch = _pitch_given(torch, pitch, dtype, rate, Co, num_frames, device)
    if mix is not None:
        mix = _second_corpus(torch, mix, _MIX, dtype, rate, Co, device)
    if reverb is not None:
        reverb = _second_corpus(torch, reverb, _REVERB, dtype, rate, Co, device)
    if level is not None:       # (what is no Level; for lufs more than 5 channels, no rate, a rate the K-weighting cannot be designed at)
        _level_checked(level, rate, Co)
        _float32(torch, dtype, "float32 crops are levelled")
    if effects is not None:
        effects = _effects_given(torch, effects, dtype, rate, device)
    if f0 is not None:
        _f0_given(torch, f0, dtype, rate, vad, num_frames)
    if normalize is not None:
        _normalize_given(torch, normalize, features, deltas, dtype, num_frames)
    if features is not None:
        _features_given(torch, features, dtype, rate, dict(deltas=deltas, normalize=normalize, vad=vad, augment=augment))
    if deltas is not None:
        if not isinstance(deltas, Deltas):
            raise ValueError(f"deltas must be a deltas.Deltas, not {deltas!r}")
        if features is None:
            raise ValueError("Deltas are derivatives of features: they need features=")
    lines = None if features is None else features.n_mels if deltas is None else deltas.lines(features.n_mels)
    if vad is not None:
        if not isinstance(vad, EnergyVad):
            raise ValueError(f"vad must be a vad.EnergyVad, not {vad!r}")
        if features is None:
            raise ValueError("an EnergyVad decides on a feature line: it needs features=")
        if vad.line >= lines:
            raise ValueError(f"vad.line {vad.line} of features with {lines} lines")
    if augment is not None:
        augment = _how(augment, "augment")
        if features is None:
            raise ValueError("a SpecAugment masks log-mel features: it needs features=")
    L = frames = None
    if any(given is not None for given in (features, mix, reverb, speed, effects, level, pitch, f0)):
        L = _frame_count("num_frames", num_frames)
        if features is not None:
            if L < features.min_frames:
                raise ValueError(features.short(L))
            frames = features.frames(L)
    return _StagePlan(speed, pitch, mix, reverb, level, effects, f0, features, deltas, vad, normalize, augment, sample_rate, mono,
                      rate, Co, L, lines, frames)


def _for_batch(plan, B, device):
    """The refusals of a checked plan that need the batch size: draws of speed=, pitch= or effects= for another number of crops,
    augment='s draws (`augment._check_draws`, whose contiguous tensors the returned plan holds) and a time warp of too many
    frames"""
    for name, pair in (("speed", plan.speed), ("pitch", plan.pitch), ("effects", plan.effects)):
        if pair is not None and pair[1] is not None:
            n = (pair[1][0] if name == "effects" else pair[1]).shape[0]
            if n != B:
                raise ValueError(f"{n} draws of {name}= for {B} crops")
    augment = plan.augment
    if augment is not None:
        if augment[1] is not None:
            plan = plan._replace(augment=(augment[0], tuple(_check_draws(augment[1], B, device))))
        if augment[0].time_warp and plan.frames > _WARP_MAX:
            raise ValueError(f"features of {plan.frames} frames: a time warp takes at most {_WARP_MAX}")
    return plan


def _middle_draws(plan, B, device, generator=None):
    """The draws of pitch=, mix=, reverb= and effects= that were not given, made in that order from `generator` (None: the
    device's default one).  speed= is drawn in front of them and augment= behind them, where their inputs are known:
    `Corpus.random_crops` needs the speed for its offsets and predicts the feat_lengths for augment=; `Corpus.crops` leaves
    the speed to `_resampled_crops` and augment= to `augment._spec_augment`."""
    pitch, mix, reverb, effects = plan.pitch, plan.mix, plan.reverb, plan.effects
    if pitch is not None and pitch[1] is None:
        pitch = (pitch[0], pitch[0].draw(B, generator=generator, device=device))
    if mix is not None and mix[1] is None:
        mix = (mix[0], mix[0].draw(B, plan.L, sample_rate=plan.rate, generator=generator))
    if reverb is not None and reverb[1] is None:
        reverb = (reverb[0], reverb[0].draw(B, generator=generator, device=device))
    if effects is not None and effects[1] is None:
        effects = (effects[0], effects[0].draw(B, plan.rate, generator=generator, device=device))
    return plan._replace(pitch=pitch, mix=mix, reverb=reverb, effects=effects)
