"""Corpus.crops(f0=PYin) and Corpus.random_crops(f0=PYin) on the GPU, on the synthetic corpus of tests/test_corpus_level.py: the
track is held bit for bit to alac.pyin of the waveform the call returns with the same arguments and draws -- natively, as one
channel at another rate, beside features, behind speed= --, a Yin on the same draws still to alac.yin, the refusals to
ValueError before any device work, and a second call to the scratch of the first."""
import pytest

from test_corpus_level import L, RATE, bits, device_crops, write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(write(pkg, torch, tmp_path_factory.mktemp("corpus_pyin"), RATE, "f0")) as c:
        yield c


def pyin_spec(pkg, rate, **kw):
    return pkg.PYin(rate, 256, 80, 100.0, 500.0, resolution=0.5, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(mono=True), dict(sample_rate=8000, mono=True)], ids=["native", "mono", "resampled-mono"])
def test_the_track_is_pyin_of_the_waveform_the_call_returns(corpus, kw):
    import torch

    import alac.net_amd as pkg

    rate = kw.get("sample_rate", RATE)
    cf, co = device_crops(torch, corpus, kw.get("sample_rate"))
    spec = pyin_spec(pkg, rate)
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    got = corpus.crops(cf, co, L, check=False, f0=spec, **kw)
    assert len(got) == 3 and torch.equal(bits(got[0]), bits(pcm)) and torch.equal(got[1], lengths)
    want = pkg.pyin(pcm, spec, lengths)
    assert tuple(got[2].shape) == (5, pcm.shape[1], 3, spec.frames(L)) and torch.equal(bits(got[2]), bits(want))
    # the crop outside the corpus is silence: one frame, the first unvoiced state, nothing behind it
    assert lengths.tolist()[-1] == -1 and not bool(got[2][-1, :, 1:].any()) and not bool(got[2][-1, :, :, 1:].any())
    assert bool(spec.voiced(got[2])[0].any()) and float(got[2][0, 0, 0].max()) > 100.0
    track = got[2].clone()
    for feat in (pkg.LogMel(rate, n_fft=256, hop_length=80, n_mels=20), pkg.KaldiFbank(rate, win_length=200, hop_length=80, n_mels=20)):
        like = pkg.PYin.like(feat, win_length=256, fmin=100.0, fmax=500.0, resolution=0.5)
        feats, flen = corpus.crops(cf, co, L, check=False, features=feat, **kw)
        feats = feats.clone()
        got = corpus.crops(cf, co, L, check=False, features=feat, f0=like, **kw)
        assert torch.equal(bits(got[0]), bits(feats)) and torch.equal(got[1], flen)
        assert got[2].shape[-1] == feats.shape[-1] and torch.equal(bits(got[2]), bits(pkg.pyin(pcm, like, lengths)))
        if like.center:
            assert like == spec and torch.equal(bits(got[2]), bits(track))
        assert torch.equal(like.lengths(lengths), flen)
    host = corpus.crops(cf[:4].tolist(), co[:4].tolist(), L, f0=spec, **kw)
    assert torch.equal(bits(host[2]), bits(track[:4]))


def test_the_track_follows_speed_and_a_yin_is_what_it_was(corpus):
    """Behind speed= the track is that of the perturbed waveform; a second call writes the scratch of the first; and a Yin on
    the same draws returns alac.yin of its waveform, as before"""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.speed import SpeedPerturb

    cf, co = device_crops(torch, corpus)
    spec, plain = pyin_spec(pkg, RATE), pkg.Yin(RATE, 256, 80, 100.0, 500.0, 0.15)
    stages = dict(speed=(SpeedPerturb(), torch.tensor([0, 1, 2, 0, 1], device="cuda", dtype=torch.int64)))
    pcm, lengths = corpus.crops(cf, co, L, check=False, **stages)
    pcm = pcm.clone()
    got = corpus.crops(cf, co, L, check=False, f0=spec, **stages)
    assert torch.equal(bits(got[0]), bits(pcm)) and torch.equal(bits(got[2]), bits(pkg.pyin(pcm, spec, lengths)))
    track = got[2].clone()
    again = corpus.crops(cf, co, L, check=False, f0=spec)[2]
    assert again.data_ptr() == got[2].data_ptr() and not torch.equal(bits(again), bits(track))
    y = corpus.crops(cf, co, L, check=False, f0=plain, **stages)
    assert tuple(y[2].shape) == (5, pcm.shape[1], 2, plain.frames(L)) and torch.equal(bits(y[2]), bits(pkg.yin(pcm, plain, lengths)))


def test_random_crops_return_the_track_of_the_crops_they_drew(corpus):
    import torch

    import alac.net_amd as pkg

    spec = pyin_spec(pkg, RATE)
    g = torch.Generator().manual_seed(11)
    pcm, lengths, files, offs, track = corpus.random_crops(6, L, generator=g, f0=spec)
    pcm, track = pcm.clone(), track.clone()
    again = corpus.crops(files, offs, L, f0=spec)
    assert torch.equal(bits(again[0]), bits(pcm)) and torch.equal(bits(again[2]), bits(track))
    g = torch.Generator().manual_seed(11)
    plain = corpus.random_crops(6, L, generator=g)           # (f0= draws nothing)
    assert len(plain) == 4 and torch.equal(plain[2], files) and torch.equal(plain[3], offs) and torch.equal(bits(plain[0]), bits(pcm))


def test_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    spec = pyin_spec(pkg, RATE)
    feat = pkg.KaldiMfcc(RATE)
    snip = pkg.PYin.like(feat)
    for kw in (dict(f0=pkg.PYin(8000)), dict(f0=spec, dtype=torch.int32), dict(f0="pyin"), dict(f0=spec.yin.threshold),
               dict(f0=snip, features=feat, vad=pkg.EnergyVad()), dict(f0=spec, sample_rate=8000)):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, check=False, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(4, L, **kw)
    with pytest.raises(ValueError):
        corpus.crops(cf, co, snip.min_frames - 1, check=False, f0=snip)
    with pytest.raises(ValueError):
        corpus.random_crops(4, snip.min_frames - 1, f0=snip)
