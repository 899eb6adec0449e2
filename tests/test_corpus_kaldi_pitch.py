"""Corpus.crops(f0=KaldiPitch) and Corpus.random_crops(f0=KaldiPitch) on the GPU, on the synthetic corpus of
tests/test_corpus_level.py (the fixtures of tests/test_corpus_pyin.py): the track is held bit for bit to alac.kaldi_pitch of the
waveform the call returns with the same arguments and draws -- natively, beside a KaldiFbank, behind effects= and mix= --, the
refusals to ValueError before any device work, and a second call to the scratch of the first."""
import pytest

from test_corpus_level import L, RATE, bits, device_crops, write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(write(pkg, torch, tmp_path_factory.mktemp("corpus_kaldi_pitch"), RATE, "kp")) as c:
        yield c


def test_the_track_is_kaldi_pitch_of_the_waveform_the_call_returns(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    feat = pkg.KaldiFbank(RATE)
    spec = pkg.KaldiPitch.like(feat)
    pcm, lengths = corpus.crops(cf, co, L, check=False)
    pcm = pcm.clone()
    got = corpus.crops(cf, co, L, check=False, f0=spec)
    assert len(got) == 3 and torch.equal(bits(got[0]), bits(pcm)) and torch.equal(got[1], lengths)
    want = pkg.kaldi_pitch(pcm, spec, lengths)
    assert tuple(got[2].shape) == (5, pcm.shape[1], 3, spec.frames(L)) and torch.equal(bits(got[2]), bits(want))
    assert lengths.tolist()[-1] == -1 and not bool(got[2][-1].any()) and bool(got[2][0].any())
    track = got[2].clone()
    mono = corpus.crops(cf, co, L, check=False, mono=True)[0].clone()
    feats, flen = corpus.crops(cf, co, L, check=False, features=feat, mono=True)
    feats = feats.clone()
    both = corpus.crops(cf, co, L, check=False, features=feat, f0=spec, mono=True)
    assert torch.equal(bits(both[0]), bits(feats)) and torch.equal(both[1], flen) and torch.equal(spec.lengths(lengths), flen)
    assert torch.equal(bits(both[2]), bits(pkg.kaldi_pitch(mono, spec, lengths)))
    assert tuple(torch.cat([both[0], both[2]], 2).shape) == (5, 1, 83, feat.frames(L))        # ESPnet's fbank_pitch
    # a second call writes the scratch of the first
    again = corpus.crops(cf.flip(0), co.flip(0), L, check=False, f0=spec)[2]
    assert again.data_ptr() == got[2].data_ptr() and not torch.equal(bits(again), bits(track))


def test_the_track_follows_effects_and_mix(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    spec = pkg.KaldiPitch(RATE, process=False)
    add = pkg.AddNoise(corpus, (5.0, 15.0))
    fx = pkg.Effects((pkg.RandomBiquad("highpass", (40.0, 120.0)),), gain=(0.125, 2.0))
    g = torch.Generator(device="cuda").manual_seed(3)
    stages = dict(mix=(add, add.draw(5, L, generator=g)), effects=(fx, fx.draw(5, RATE, generator=g)))
    pcm, lengths = corpus.crops(cf, co, L, check=False, **stages)
    pcm = pcm.clone()
    got = corpus.crops(cf, co, L, check=False, f0=spec, **stages)
    assert torch.equal(bits(got[0]), bits(pcm)) and torch.equal(bits(got[2]), bits(pkg.kaldi_pitch(pcm, spec, lengths)))
    assert tuple(got[2].shape) == (5, pcm.shape[1], 2, spec.frames(L))


def test_random_crops_return_the_track_of_the_crops_they_drew(corpus):
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiPitch(RATE)
    g = torch.Generator().manual_seed(11)
    pcm, lengths, files, offs, track = corpus.random_crops(6, L, generator=g, f0=spec)
    pcm, track = pcm.clone(), track.clone()
    assert torch.equal(bits(track), bits(pkg.kaldi_pitch(pcm, spec, lengths)))
    again = corpus.crops(files, offs, L, f0=spec)
    assert torch.equal(bits(again[0]), bits(pcm)) and torch.equal(bits(again[2]), bits(track))


def test_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    feat = pkg.KaldiMfcc(RATE)
    spec = pkg.KaldiPitch.like(feat)
    for kw in (dict(f0=pkg.KaldiPitch(8000)), dict(f0=spec, dtype=torch.int32), dict(f0=spec, features=feat, vad=pkg.EnergyVad()),
               dict(f0=spec, sample_rate=8000)):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, check=False, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(4, L, **kw)
    with pytest.raises(ValueError, match="f0 must be a yin.Yin or a pyin.PYin, not 440"):
        corpus.crops(cf, co, L, check=False, f0=440)
    with pytest.raises(ValueError):
        corpus.crops(cf, co, spec.min_frames - 1, check=False, f0=spec)
