"""Corpus.crops(f0=) and Corpus.random_crops(f0=) on the GPU, on the synthetic corpus of tests/test_corpus_level.py: the track is
held bit for bit to alac.yin of the waveform the call returns with the same arguments and draws -- natively, as one channel at
another rate, beside features and behind the waveform stages --, the generator to the crops it drew, the refusals to ValueError
before any device work, and, end to end, a pitch shift of +2 and -2 semitones to +200 and -200 cents of measured F0."""
import numpy as np
import pytest

from test_corpus_level import L, RATE, bits, device_crops, write

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(write(pkg, torch, tmp_path_factory.mktemp("corpus_yin"), RATE, "f0")) as c:
        yield c


@pytest.mark.parametrize("kw", [dict(), dict(mono=True), dict(sample_rate=8000, mono=True)], ids=["native", "mono", "resampled-mono"])
def test_the_track_is_yin_of_the_waveform_the_call_returns(corpus, kw):
    import torch

    import alac.net_amd as pkg

    rate = kw.get("sample_rate", RATE)
    cf, co = device_crops(torch, corpus, kw.get("sample_rate"))
    spec = pkg.Yin(rate, 256, 80, 100.0, 500.0, 0.15)
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    got = corpus.crops(cf, co, L, check=False, f0=spec, **kw)
    assert len(got) == 3 and torch.equal(bits(got[0]), bits(pcm)) and torch.equal(got[1], lengths)
    want = pkg.yin(pcm, spec, lengths)
    assert tuple(got[2].shape) == (5, pcm.shape[1], 2, spec.frames(L)) and torch.equal(bits(got[2]), bits(want))
    assert lengths.tolist()[-1] == -1 and got[2][-1, :, :, 0].tolist() == [[0.0, 1.0]] * pcm.shape[1] and not bool(got[2][-1, :, :, 1:].any())
    assert bool(spec.voiced(got[2])[0].any()) and float(got[2][0, 0, 0].max()) > 100.0
    track = got[2].clone()
    # beside features the track is the same, in the frames of the features, and the features are what they were
    for feat in (pkg.LogMel(rate, n_fft=256, hop_length=80, n_mels=20), pkg.KaldiFbank(rate, win_length=200, hop_length=80, n_mels=20)):
        like = pkg.Yin.like(feat, win_length=256, fmin=100.0, fmax=500.0, threshold=0.15)
        feats, flen = corpus.crops(cf, co, L, check=False, features=feat, **kw)
        feats = feats.clone()
        got = corpus.crops(cf, co, L, check=False, features=feat, f0=like, **kw)
        assert torch.equal(bits(got[0]), bits(feats)) and torch.equal(got[1], flen)
        assert got[2].shape[-1] == feats.shape[-1] and torch.equal(bits(got[2]), bits(pkg.yin(pcm, like, lengths)))
        if like.center:
            assert like == spec and torch.equal(bits(got[2]), bits(track))
        assert torch.equal(like.lengths(lengths), flen)
    # host indices give the same crops and the same track
    host = corpus.crops(cf[:4].tolist(), co[:4].tolist(), L, f0=spec, **kw)
    assert torch.equal(bits(host[2]), bits(track[:4]))


def test_the_track_follows_the_waveform_stages(corpus):
    """Behind level= and effects= the track is that of the levelled and filtered waveform"""
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    spec = pkg.Yin(RATE, 256, 80, 100.0, 500.0)
    eff = pkg.Effects.telephone()
    draws = eff.draw(5, RATE, device="cuda")
    stages = dict(level=pkg.Level.rms(-25.0), effects=(eff, draws))
    pcm, lengths = corpus.crops(cf, co, L, check=False, **stages)
    pcm = pcm.clone()
    got = corpus.crops(cf, co, L, check=False, f0=spec, **stages)
    assert torch.equal(bits(got[0]), bits(pcm)) and torch.equal(bits(got[2]), bits(pkg.yin(pcm, spec, lengths)))
    track = got[2].clone()                          # (the track is a view of the corpus's scratch: the next call writes it again)
    plain = corpus.crops(cf, co, L, check=False, f0=spec)[2]
    assert plain.data_ptr() == got[2].data_ptr() and not torch.equal(bits(plain), bits(track))


def test_random_crops_return_the_track_of_the_crops_they_drew(corpus):
    import torch

    import alac.net_amd as pkg

    spec = pkg.Yin(RATE, 256, 80, 100.0, 500.0)
    g = torch.Generator().manual_seed(11)
    pcm, lengths, files, offs, track = corpus.random_crops(6, L, generator=g, f0=spec)
    pcm, track = pcm.clone(), track.clone()
    again = corpus.crops(files, offs, L, f0=spec)
    assert torch.equal(bits(again[0]), bits(pcm)) and torch.equal(bits(again[2]), bits(track))
    g = torch.Generator().manual_seed(11)
    plain = corpus.random_crops(6, L, generator=g)
    assert len(plain) == 4 and torch.equal(plain[2], files) and torch.equal(plain[3], offs) and torch.equal(bits(plain[0]), bits(pcm))


def test_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    spec = pkg.Yin(RATE, 256, 80, 100.0, 500.0)
    feat = pkg.KaldiMfcc(RATE)
    snip = pkg.Yin.like(feat)
    for kw in (dict(f0=pkg.Yin(8000)), dict(f0=spec, dtype=torch.int32), dict(f0="yin"), dict(f0=spec.threshold),
               dict(f0=snip, features=feat, vad=pkg.EnergyVad()), dict(f0=spec, sample_rate=8000)):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, check=False, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(4, L, **kw)
    with pytest.raises(ValueError):
        corpus.crops(cf, co, snip.min_frames - 1, check=False, f0=snip)
    with pytest.raises(ValueError):
        corpus.random_crops(4, snip.min_frames - 1, f0=snip)


def test_a_pitch_shift_of_two_semitones_moves_the_measured_f0_by_200_cents():
    """The tolerance: the float64 pair pitch_shift_host then yin_host on this tone, measured on the CPU while this was written,
    is 0.098 cents above +200 and 0.054 cents above -200 in the median over the voiced inner frames; to the larger is added
    the module's float32 bound on f0 (yin.f0_bound) at the shorter of the two lags, 95, with kappa = 300 -- above what any
    frame of such a tone has (266 on the noisier signal of tests/test_yin_spec.py) --: 0.43 cents.  0.53 cents in all."""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.yin import f0_bound

    n = np.arange(8000)
    ph = 2 * np.pi * 150 * n / RATE
    x = (0.5 * np.sin(ph) + 0.3 * np.sin(2 * ph) + 0.2 * np.sin(3 * ph)).astype(np.float32)
    spec = pkg.Yin(RATE)
    tol = 0.098 + 1200.0 * np.log2(1.0 + float(f0_bound(spec, 95, 300.0)))
    assert 0.5 < tol < 0.56
    shift = pkg.PitchShift(semitones=(-2, 2))
    with pkg.Corpus.from_pcm(torch.from_numpy(x[None, None, :]).cuda(), [8000], sample_rate=RATE) as c:
        files, offs = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        pcm, lengths, track = c.crops(files, offs, 8000, pitch=(shift, torch.tensor([1, 0], device="cuda")), f0=spec)
        inner = slice(6, track.shape[-1] - 6)
        for b, want in ((0, 200.0), (1, -200.0)):
            voiced = spec.voiced(track)[b, 0, inner]
            cents = pkg.hz_to_cents(track[b, 0, 0, inner][voiced].double(), 150.0).cpu().numpy()
            print(want, "cents: median", float(np.median(cents)), "over", int(voiced.sum()), "voiced frames")
            assert int(voiced.sum()) >= 30 and abs(float(np.median(cents)) - want) <= tol
