"""The one check of the stage keywords of a crop step (alac.net_amd/_cropstages.py), without a device: every refusal that
`Corpus.crops` and `Corpus.random_crops` have in front of their device work, by its message; the record an accepted call gets;
which of two faults is reported; the refusals that need the batch size; the order of the middle draws; and that `crops` and
`random_crops` run the check once and their shared body never.  The facts of a call are plain values, the draws host tensors,
and a second corpus is a `Corpus` that was never opened: the check asks it for `_gpu`, `_dev` and `channels` only."""
import re

import pytest

RATE, L = 16000, 2500


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def pkg():
    import alac.net_amd as pkg

    return pkg


def standin(pkg, torch, channels=1, device="cpu"):
    class Standin(pkg.Corpus):
        def __init__(self):
            self._gpu, self._pinned, self._dev, self.channels = type("Open", (), dict(close=lambda self: None))(), None, torch.device(device), channels

    return Standin()


def plan(torch, channels=2, own_rate=RATE, device="cpu", dtype=None, num_frames=L, sample_rate=None, mono=False, **keywords):
    from alac.net_amd._cropstages import _stage_plan

    return _stage_plan(channels, own_rate, torch.device(device), dtype, num_frames, sample_rate, mono, **keywords)


def refusals(pkg, torch):
    """(what is refused, the message, the call's facts and keywords) for every raise `crops`, `random_crops` and the `_*_given`
    methods had in front of the batch size"""
    i64, f64 = (lambda *s: torch.zeros(s, dtype=torch.int64)), (lambda *s: torch.zeros(s, dtype=torch.float64))
    i32 = dict(dtype=torch.int32)
    sp, ps, fx = pkg.SpeedPerturb(), pkg.PitchShift(), pkg.Effects.telephone()
    noise, rirs, wide, far = standin(pkg, torch), standin(pkg, torch, 2), standin(pkg, torch), standin(pkg, torch, device="meta")
    add, aug = pkg.AddNoise(noise, 10), pkg.Reverb(rirs)
    closed = (pkg.AddNoise(standin(pkg, torch), 10), pkg.Reverb(standin(pkg, torch)))
    closed[0].noise._gpu = closed[1].rirs._gpu = None
    add_wide, aug_wide = pkg.AddNoise(wide, 10), pkg.Reverb(wide)
    wide.channels = 3
    room = pkg.Reverb(pkg.ShoeboxRooms(), max_seconds=0.1)
    rdraws = (f64(4, 9), torch.zeros(4, 6), torch.zeros(4, dtype=torch.bool))
    mel, fbank, yin = pkg.LogMel(RATE), pkg.KaldiFbank(RATE), pkg.Yin(RATE, center=False, align_length=400)
    energies, pcen = pkg.LogMel(RATE, log=None), pkg.Pcen(frame_rate=100.0)
    return [
        ("speed: no SpeedPerturb", "speed must be a speed.SpeedPerturb or (SpeedPerturb, what its draw() returned), not 3", dict(speed=3)),
        ("speed: a triple", "speed must be a speed.SpeedPerturb or", dict(speed=(sp, i64(4), 1))),
        ("speed: int32", "float32 crops are speed-perturbed", dict(speed=sp, **i32)),
        ("speed: channels", "3 channels: the resampler takes 1 or 2", dict(speed=sp, channels=3, mono=True)),
        ("speed: no rate", "differ in sample rate: crops need sample_rate=", dict(speed=sp, own_rate=None)),
        ("speed: float draws", "the draws of speed= must be the integer tensor [B] of SpeedPerturb.draw on cpu", dict(speed=(sp, f64(4)))),
        ("speed: draws [B, 1]", "the draws of speed= must be the integer tensor", dict(speed=(sp, i64(4, 1)))),
        ("speed: draws elsewhere", "the draws of speed= must be the integer tensor", dict(speed=(sp, i64(4)), device="meta")),
        ("pitch: no PitchShift", "pitch must be a pitch.PitchShift or (PitchShift, what its draw() returned), not 'up'", dict(pitch="up")),
        ("pitch: int32", "float32 crops are pitch-shifted", dict(pitch=ps, **i32)),
        ("pitch: channels", "3 channels: the resampler behind the vocoder takes 1 or 2", dict(pitch=ps, channels=3)),
        ("pitch: no rate", "differ in sample rate: crops need sample_rate=", dict(pitch=ps, own_rate=None)),
        ("pitch: short", "crops of 256 frames: a PitchShift of n_fft 512 reflects 256 and needs more", dict(pitch=ps, num_frames=256)),
        ("pitch: bool draws", "the draws of pitch= must be the integer tensor [B] of PitchShift.draw on cpu",
         dict(pitch=(ps, torch.zeros(4, dtype=torch.bool)))),
        ("mix: no AddNoise", "mix must be a mix.AddNoise or (AddNoise, what its draw() returned), not", dict(mix=aug)),
        ("mix: two tensors", "the draws of mix= must be the three tensors (noise_files, noise_offsets, snr_db) of AddNoise.draw",
         dict(mix=(add, (i64(4), i64(4))))),
        ("mix: integer ratios", "the draws of mix= must be the three tensors", dict(mix=(add, (i64(4), i64(4), i64(4))))),
        ("mix: lengths differ", "the draws of mix= must be the three tensors", dict(mix=(add, (i64(4), i64(3), torch.zeros(4))))),
        ("mix: draws elsewhere", "the draws of mix= must be on meta", dict(mix=(pkg.AddNoise(far, 10), (i64(4), i64(4), torch.zeros(4))), device="meta")),
        ("mix: int32", "noise is mixed into float32 crops", dict(mix=add, **i32)),
        ("mix: closed", "the noise corpus is closed", dict(mix=closed[0])),
        ("mix: another device", "the noise corpus is on meta, the crops on cpu", dict(mix=pkg.AddNoise(far, 10))),
        ("mix: no rate", "crops need sample_rate=, and the noise a rate to crop at", dict(mix=add, own_rate=None)),
        ("mix: channels", "a noise corpus of 3 channels into crops of 2: it can become one channel from 1 or 2 only", dict(mix=add_wide)),
        ("reverb: no Reverb", "reverb must be a reverb.Reverb or (Reverb, what its draw() returned), not", dict(reverb=add)),
        ("reverb: float files", "the draws of reverb= must be the two tensors (rir_files, keep) of Reverb.draw",
         dict(reverb=(aug, (f64(4), torch.zeros(4, dtype=torch.bool))))),
        ("reverb: keep not bool", "the draws of reverb= must be the two tensors", dict(reverb=(aug, (i64(4), i64(4))))),
        ("reverb: draws elsewhere", "the draws of reverb= must be on meta",
         dict(reverb=(pkg.Reverb(far), (i64(4), torch.zeros(4, dtype=torch.bool))), device="meta")),
        ("reverb: int32", "float32 crops are reverberated", dict(reverb=aug, **i32)),
        ("reverb: closed", "the corpus of impulse responses is closed", dict(reverb=closed[1])),
        ("reverb: another device", "the corpus of impulse responses is on meta, the crops on cpu", dict(reverb=pkg.Reverb(far))),
        ("reverb: no rate", "crops need sample_rate=, and the responses a rate to crop at", dict(reverb=aug, own_rate=None)),
        ("reverb: channels", "impulse responses of 3 channels into crops of 2: they can become one channel from 1 or 2 only", dict(reverb=aug_wide)),
        ("rooms: two tensors", "the draws of reverb= must be the three tensors (geometry, beta, keep) of Reverb.draw", dict(reverb=(room, rdraws[:2]))),
        ("rooms: geometry float32", "the draws of reverb= must be the three tensors", dict(reverb=(room, (rdraws[0].float(),) + rdraws[1:]))),
        ("rooms: draws elsewhere", "the draws of reverb= must be on meta", dict(reverb=(room, rdraws), device="meta")),
        ("rooms: int32", "float32 crops are reverberated", dict(reverb=room, **i32)),
        ("rooms: no rate", "crops need sample_rate=, and the responses a rate to be computed at", dict(reverb=room, own_rate=None)),
        ("level: no Level", "level must be a level.Level, not -20", dict(level=-20)),
        ("level: loudness of 6 channels", "6 channels: BS.1770 weighs at most 5", dict(level=pkg.Level("lufs", -23.0), channels=6)),
        ("level: int32", "float32 crops are levelled", dict(level=pkg.Level("rms", -20.0), **i32)),
        ("effects: no Effects", "effects must be a biquad.Effects or (Effects, what its draw() returned), not 'phone'", dict(effects="phone")),
        ("effects: int32", "float32 crops are filtered", dict(effects=fx, **i32)),
        ("effects: no rate", "differ in sample rate: crops need sample_rate=", dict(effects=fx, own_rate=None)),
        ("effects: Nyquist", "a lowpass at up to 3400.0 Hz on crops at 6000 Hz: at or above Nyquist", dict(effects=fx, sample_rate=6000)),
        ("effects: sections", "the draws of effects= must be the two float64 tensors (coeffs [B, 4, 5], gain [B]) of Effects.draw",
         dict(effects=(fx, (f64(4, 3, 5), f64(4))))),
        ("effects: float32 gain", "the draws of effects= must be the two float64 tensors", dict(effects=(fx, (f64(4, 4, 5), torch.zeros(4))))),
        ("effects: draws elsewhere", "the draws of effects= must be on meta", dict(effects=(fx, (f64(4, 4, 5), f64(4))), device="meta")),
        ("f0: no Yin", "f0 must be a yin.Yin or a pyin.PYin, not 440", dict(f0=440)),
        ("f0: no rate", "differ in sample rate: crops need sample_rate=", dict(f0=yin, own_rate=None)),
        ("f0: another rate", "f0 for 16000 Hz, crops at 8000 Hz", dict(f0=yin, sample_rate=8000)),
        ("f0: int32", "F0 is estimated from float32 crops", dict(f0=yin, **i32)),
        ("f0: with vad", "f0= with vad=: the selected frames would no longer line up with the track", dict(f0=yin, features=mel, vad=pkg.EnergyVad())),
        ("f0: short", "num_frames 399: a row of fewer than 400 frames has no F0 frame", dict(f0=yin, num_frames=399)),
        ("normalize: another type", "normalize must be a normalize.MeanVar, a normalize.TopDb, a sliding.SlidingMeanVar or a pcen.Pcen, not 'cmvn'",
         dict(normalize="cmvn")),
        ("normalize: a Pcen of PCM", "a Pcen compresses mel or constant-Q energies: it needs features=", dict(normalize=pcen)),
        ("normalize: a Pcen of logs", "a Pcen compresses energies: features with log=None", dict(normalize=pcen, features=mel)),
        ("normalize: a Pcen of cepstra", "a Pcen compresses energies: features with log=None", dict(normalize=pcen, features=pkg.KaldiMfcc(RATE))),
        ("normalize: a Pcen with deltas", "a Pcen compresses energies: deltas= of them are none", dict(normalize=pcen, features=energies, deltas=pkg.Deltas())),
        ("normalize: a Pcen of 40 lines", "a Pcen with 40 values per parameter, features with 80 lines",
         dict(normalize=pkg.Pcen(frame_rate=100.0, gain=[0.9] * 40), features=energies)),
        ("normalize: a TopDb of PCM", "a TopDb clamps log-mel features: it needs features=", dict(normalize=pkg.TopDb())),
        ("normalize: int32 PCM", "a MeanVar normalises float32 crops", dict(normalize=pkg.MeanVar(), **i32)),
        ("normalize: a wide window on long PCM", "lines of 16385 frames: above 16384 a sliding window takes at most 7648 frames",
         dict(normalize=pkg.SlidingMeanVar(window=7649), num_frames=16385)),
        ("normalize: a wide window on long features", "lines of 16385 frames: above 16384 a sliding window takes at most 7648 frames",
         dict(normalize=pkg.SlidingMeanVar(window=7649), features=pkg.LogMel(RATE, 400, 1, 80), num_frames=16384)),
        ("features: another type", "features must be a features.LogMel or a fbank.KaldiFbank or a mfcc.KaldiMfcc or a cqt.ConstantQ or a "
         "stft.Spectrogram, not 16000 (sample_rate= and mono= go by keyword)", dict(features=16000)),
        ("features: no rate", "differ in sample rate: crops need sample_rate=", dict(features=mel, own_rate=None)),
        ("features: another rate", "features for 16000 Hz, crops at 8000 Hz", dict(features=mel, sample_rate=8000)),
        ("features: int32", "features are computed from float32 crops", dict(features=mel, **i32)),
        ("features: a complex spectrum with augment", "a Spectrogram with power=None gives real and imaginary parts: augment= takes magnitudes",
         dict(features=pkg.Spectrogram(RATE, power=None), augment=pkg.SpecAugment())),
        ("features: short", "num_frames 399: a row of fewer than 400 frames has no feature frame", dict(features=fbank, num_frames=399)),
        ("deltas: another type", "deltas must be a deltas.Deltas, not 2", dict(deltas=2, features=mel)),
        ("deltas: of PCM", "Deltas are derivatives of features: they need features=", dict(deltas=pkg.Deltas())),
        ("vad: another type", "vad must be a vad.EnergyVad, not True", dict(vad=True, features=mel)),
        ("vad: of PCM", "an EnergyVad decides on a feature line: it needs features=", dict(vad=pkg.EnergyVad())),
        ("vad: line", "vad.line 240 of features with 240 lines", dict(vad=pkg.EnergyVad(line=240), features=mel, deltas=pkg.Deltas())),
        ("augment: another type", "augment must be a SpecAugment or the pair (SpecAugment, draws), not (1, 2, 3)", dict(augment=(1, 2, 3), features=mel)),
        ("augment: of PCM", "a SpecAugment masks log-mel features: it needs features=", dict(augment=pkg.SpecAugment())),
    ]


def test_every_refusal_in_front_of_the_batch_size(pkg, torch):
    cases = refusals(pkg, torch)
    assert len(cases) == 77 and len({name for name, _, _ in cases}) == 77
    for name, message, call in cases:
        with pytest.raises(ValueError, match=re.escape(message)):
            plan(torch, **call)
            pytest.fail(f"{name}: accepted")


def test_the_record_of_an_accepted_call(pkg, torch):
    from alac.net_amd._cropstages import _StagePlan

    assert plan(torch) == _StagePlan(*[None] * 12, sample_rate=None, mono=False, rate=RATE, Co=2, L=None, lines=None, frames=None)
    # a bare specification becomes (specification, None), a pair stays; the others stay as they are
    sp, ps, fx, sa = pkg.SpeedPerturb(), pkg.PitchShift(), pkg.Effects.telephone(), pkg.SpecAugment()
    add, aug = pkg.AddNoise(standin(pkg, torch, 2), 10), pkg.Reverb(standin(pkg, torch, 2))
    room = pkg.Reverb(pkg.ShoeboxRooms(), max_seconds=0.1)
    mel, dl, vad, how, lv, yin = pkg.LogMel(8000), pkg.Deltas(), pkg.EnergyVad(line=239), pkg.MeanVar(), pkg.Level("rms", -20.0), pkg.Yin(8000)
    got = plan(torch, channels=3, own_rate=None, sample_rate=8000, mono=True, mix=add, reverb=room, level=lv, effects=fx, features=mel,
               deltas=dl, vad=vad, normalize=how, augment=sa)
    assert got == _StagePlan(None, None, (add, None), (room, None), lv, (fx, None), None, mel, dl, vad, how, (sa, None), 8000, True,
                             rate=8000, Co=1, L=L, lines=240, frames=mel.frames(L))
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)
    draws = dict(speed=i64(4), pitch=i64(5), mix=(i64(4), i64(4), torch.zeros(4)), reverb=(i64(4), torch.zeros(4, dtype=torch.bool)),
                 effects=(torch.zeros(4, 4, 5, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)),
                 augment=(None, torch.zeros(4, 2, 2, dtype=torch.int32), torch.zeros(4, 2, 2, dtype=torch.int32)))
    specs = dict(speed=sp, pitch=ps, mix=pkg.AddNoise(standin(pkg, torch, 2), 10), reverb=aug, effects=fx, augment=sa)
    got = plan(torch, f0=yin, sample_rate=8000, features=mel, **{k: (specs[k], draws[k]) for k in specs})
    for k in specs:
        assert getattr(got, k)[0] is specs[k] and getattr(got, k)[1] is draws[k], k
    assert (got.f0, got.Co, got.L, got.lines, got.frames) == (yin, 2, L, 80, mel.frames(L))
    # L is there for the stages in front of the waveform and for features, not for normalize= alone
    assert plan(torch, normalize=how).L is None and plan(torch, level=lv).L == L and plan(torch, level=lv).frames is None
    rooms = (torch.zeros(4, 9, dtype=torch.float64), torch.zeros(4, 6), torch.zeros(4, dtype=torch.bool))
    assert plan(torch, reverb=(room, rooms)).reverb == (room, rooms)


def test_of_two_faults_the_first_in_stage_order_is_reported(pkg, torch):
    mel = pkg.LogMel(RATE)
    for first, both in (("speed must be", dict(speed=1, pitch=2)),                                      # speed, pitch
                        ("float32 crops are levelled", dict(level=pkg.Level("rms", -20.0), effects=pkg.Effects.telephone(), dtype=torch.int32)),
                        ("normalize must be", dict(normalize=1, features=2)),                           # normalize, features
                        ("deltas must be", dict(features=mel, deltas=1, vad=pkg.EnergyVad(line=80))),   # deltas, vad
                        ("vad must be", dict(features=mel, vad=1, augment=1)),                          # vad, augment
                        ("augment must be", dict(features=pkg.KaldiFbank(RATE), augment=1, num_frames=10))):    # augment, the length
        with pytest.raises(ValueError, match=first):
            plan(torch, **both)


def test_the_refusals_that_need_the_batch_size(pkg, torch):
    from alac.net_amd._cropstages import _for_batch

    cpu = torch.device("cpu")
    i64, i32 = (lambda *s: torch.zeros(s, dtype=torch.int64)), (lambda *s: torch.zeros(s, dtype=torch.int32))
    sp, ps, fx, sa, mel = pkg.SpeedPerturb(), pkg.PitchShift(), pkg.Effects.telephone(), pkg.SpecAugment(time_warp=3), pkg.LogMel(RATE)
    edraws = (torch.zeros(5, 4, 5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64))
    for message, call in (("3 draws of speed= for 4 crops", dict(speed=(sp, i64(3)), pitch=(ps, i64(5)))),
                          ("5 draws of pitch= for 4 crops", dict(pitch=(ps, i64(5)), effects=(fx, edraws))),
                          ("5 draws of effects= for 4 crops", dict(effects=(fx, edraws), features=mel, augment=(sa, (None, i32(3, 2, 2), i32(4, 2, 2))))),
                          ("the freq draws must be an int32 tensor [4, masks, 2]", dict(features=mel, augment=(sa, (None, i32(3, 2, 2), i32(4, 2, 2))))),
                          ("features of 16385 frames: a time warp takes at most 16384", dict(features=pkg.LogMel(RATE, 400, 1, 80), augment=sa, num_frames=16384))):
        checked = plan(torch, **call)
        with pytest.raises(ValueError, match=re.escape(message)):
            _for_batch(checked, 4, cpu)
    # what passes comes back as it was, the draws of augment= contiguous
    wide = i32(4, 2, 4)[:, :, ::2]
    checked = plan(torch, speed=(sp, i64(4)), features=mel, augment=(sa, (i32(4, 2), wide, i32(4, 0, 2))))
    got = _for_batch(checked, 4, cpu)
    assert got.augment[1][1].is_contiguous() and not wide.is_contiguous() and got._replace(augment=None) == checked._replace(augment=None)
    assert _for_batch(plan(torch), 4, cpu) == plan(torch)


def test_the_middle_draws_are_pitch_mix_reverb_effects(pkg, torch):
    """... from one generator in that order, each by its own `draw`; what was given stays"""
    from alac.net_amd._cropstages import _middle_draws

    cpu = torch.device("cpu")
    ps, fx = pkg.PitchShift(), pkg.Effects(pkg.RandomBiquad("peaking", (200.0, 6000.0), q=(0.5, 2.0), gain_db=(-3.0, 0.0)), gain=(0.5, 2.0))
    room = pkg.Reverb(pkg.ShoeboxRooms(), p=0.5, max_seconds=0.1)
    g = torch.Generator().manual_seed(7)
    got = _middle_draws(plan(torch, pitch=ps, reverb=room, effects=fx), 4, cpu, g)
    g = torch.Generator().manual_seed(7)
    want = (ps.draw(4, generator=g, device=cpu), room.draw(4, generator=g, device=cpu), fx.draw(4, RATE, generator=g, device=cpu))
    assert torch.equal(got.pitch[1], want[0]) and all(torch.equal(a, b) for a, b in zip(got.reverb[1] + got.effects[1], want[1] + want[2]))
    assert (got.pitch[0], got.reverb[0], got.effects[0], got.mix) == (ps, room, fx, None)
    given = torch.ones(4, dtype=torch.int64)
    g = torch.Generator().manual_seed(7)
    got = _middle_draws(plan(torch, pitch=(ps, given), effects=fx), 4, cpu, g)
    g = torch.Generator().manual_seed(7)
    assert got.pitch[1] is given and torch.equal(got.effects[1][0], fx.draw(4, RATE, generator=g, device=cpu)[0])


def test_crops_and_random_crops_check_once_and_their_body_never(pkg, torch, monkeypatch):
    """A corpus that was never opened, with a waveform of zeros: the calls go through the check and the shared body on the host"""
    from alac.net_amd import _cropstages, corpus

    seen = []

    class Plain(pkg.Corpus):
        def __init__(self):
            self._gpu, self._pinned, self._dev, self.channels, self.sample_rate, self.num_files = None, None, torch.device("cpu"), 2, RATE, 3
            self._d_num_frames = torch.tensor([30000, 24000, 9000])

        def _waveform(self, files, frame_offsets, num_frames, dtype, out, check, sample_rate, mono, speed=None):
            seen.append((files, frame_offsets, num_frames))
            return torch.zeros(len(files), 2, num_frames), torch.full((len(files),), num_frames)

    counts = dict(plan=0, batch=0)

    def counted(name, fn):
        def wrapper(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(corpus, "_stage_plan", counted("plan", _cropstages._stage_plan))
    monkeypatch.setattr(corpus, "_for_batch", counted("batch", _cropstages._for_batch))
    c = Plain()
    pcm, lengths = c.crops([0, 2], [5, 7], 100)
    assert pcm.shape == (2, 2, 100) and counts == dict(plan=1, batch=0) and seen[-1] == ([0, 2], [5, 7], 100)
    pcm, lengths, files, offs = c.random_crops(4, 100, generator=torch.Generator().manual_seed(1))
    assert pcm.shape == (4, 2, 100) and counts == dict(plan=2, batch=0) and seen[-1][0] is files and seen[-1][1] is offs
    checked = _cropstages._stage_plan(2, RATE, c._dev, None, 100)
    assert c._run(checked, [1], [0], 100, None, None, None, True)[0].shape == (1, 2, 100) and counts == dict(plan=2, batch=0)
    # a refusal of the check comes before random_crops draws: the generator stays where it was
    g = torch.Generator().manual_seed(1)
    before = g.get_state().clone()
    with pytest.raises(ValueError, match="normalize must be"):
        c.random_crops(4, 100, generator=g, normalize="cmvn")
    assert torch.equal(g.get_state(), before) and counts == dict(plan=3, batch=0)
