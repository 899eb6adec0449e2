"""Corpus.crops(pitch=) and Corpus.random_crops(pitch=) on the GPU, on a synthetic corpus of four short files written with
`save`: the stage's place in a step.  What the kernels compute is tests/test_stretch.py's subject; here crops with pitch= are held
bit for bit to alac.pitch_shift of the crops without it -- natively, with sample_rate= and mono=, behind speed= and in front of
reverb=, mix= and a KaldiFbank --, draws of the ratio 1 to the call without pitch=, a seeded generator to itself and, without
pitch=, to the draws it made before, and the refusals to ValueError before any device work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
RATE = 16000
FILES = [(9000, 16, 4096, 1, 0.3), (5001, 24, 1024, 2, 0.1), (7000, 16, 1024, 3, 0.2), (4000, 16, 4096, 4, 0.05)]


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    d = tmp_path_factory.mktemp("corpus_pitch")
    paths = []
    for i, (frames, size, fl, seed, amp) in enumerate(FILES):
        rng = np.random.default_rng(seed)
        t = np.arange(frames) / RATE
        x = np.stack([amp * np.sin(2 * np.pi * (200.0 + 150 * seed) * t + c) + 0.1 * amp * rng.standard_normal(frames) for c in (0, 1)])
        paths.append(str(d / f"p{i}.m4a"))
        pkg.save(paths[-1], torch.from_numpy(x.astype(np.float32)).cuda(), RATE, sample_size=size, frame_length=fl)
    with pkg.Corpus(paths) as c:
        yield c


def device_crops(torch, corpus, sample_rate=None):
    """A start, a middle, one that runs off its file's end, one that keeps 200 frames (too few to reflect), one outside"""
    totals = corpus.num_frames if sample_rate is None else corpus.resampled_frames(sample_rate)
    cf = [0, 1, 2, 3, 0, corpus.num_files]
    co = [0, 1000, int(totals[2]) - L // 2, int(totals[3]) - 200, 17, 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


def policy(pkg, torch):
    spec = pkg.PitchShift()
    draws = torch.tensor([0, 4, 1, 3, spec.one, 0], device="cuda")
    return spec, draws


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=8000, mono=True)], ids=["native", "resampled-mono"])
def test_crops_with_pitch_are_the_pitch_shift_of_the_crops(corpus, kw):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus, kw.get("sample_rate"))
    rate = kw.get("sample_rate", RATE)
    spec, draws = policy(pkg, torch)
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    ratios = [spec.ratios[k] for k in draws.tolist()]
    want = pkg.pitch_shift(pcm, ratios, rate, lengths, spec.n_fft)
    got, glen = corpus.crops(cf, co, L, check=False, pitch=(spec, draws), **kw)
    assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(want))
    assert lengths.tolist()[3] == 200 and lengths.tolist()[-1] == -1 and bool((got[-1] == 0).all())
    for b in (0, 1, 2):
        assert not torch.equal(bits(got[b]), bits(pcm[b])), b
    for b in (3, 4, 5):                                   # too short, the ratio 1, outside the corpus
        assert torch.equal(bits(got[b]), bits(pcm[b])), b
    v = lengths.tolist()[2]
    assert 0 < v < L and bool((got[2, :, v:] == 0).all())           # zeros stay behind the lengths
    # the ratio 1 for every crop is the call without pitch=
    ones = torch.full((6,), spec.one, device="cuda")
    same, _ = corpus.crops(cf, co, L, check=False, pitch=(spec, ones), **kw)
    assert torch.equal(bits(same), bits(pcm))
    # host indices give the same crops; behind it the features see the shifted waveform
    host = corpus.crops(cf[:5].tolist(), co[:5].tolist(), L, pitch=(spec, draws[:5]), **kw)
    assert torch.equal(bits(host[0]), bits(want[:5]))
    feat = pkg.KaldiFbank(rate, n_mels=23)
    feats, flen = corpus.crops(cf, co, L, check=False, pitch=(spec, draws), features=feat, **kw)
    assert torch.equal(bits(feats), bits(pkg.fbank(want, feat)))


def test_the_order_is_speed_pitch_reverb_mix(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    spec, draws = policy(pkg, torch)
    ratios = [spec.ratios[k] for k in draws.tolist()]
    add, rev, sp = pkg.AddNoise(corpus, (5.0, 15.0)), pkg.Reverb(corpus, max_seconds=0.02), pkg.SpeedPerturb()
    g = torch.Generator(device="cuda").manual_seed(3)
    nd, rd, sd = add.draw(6, L, generator=g), rev.draw(6, generator=g), sp.draw(6, generator=g)
    co = torch.minimum(co, torch.tensor(3000, device="cuda"))       # (inside every file at every factor)
    pcm, lengths = corpus.crops(cf, co, L, check=False, speed=(sp, sd))
    shifted = pkg.pitch_shift(pcm.clone(), ratios, RATE, lengths)
    got, glen = corpus.crops(cf, co, L, check=False, speed=(sp, sd), pitch=(spec, draws))
    assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(shifted))
    # the source's pitch changes, not the room's: reverb and mix see the shifted waveform
    room = corpus.crops(cf, co, L, check=False, speed=(sp, sd), pitch=(spec, draws), reverb=(rev, rd), mix=(add, nd))[0].clone()
    rir, rl = corpus.crops(rd[0], torch.zeros(6, dtype=torch.int64, device="cuda"), rev.frames(RATE), check=False)
    rir, rl = rir.clone(), torch.where(rd[1], rl, 0)
    noise, nl = corpus.crops(nd[0], nd[1], L, check=False)
    by_hand = pkg.mix(pkg.reverb(shifted, rir, lengths, rl), noise.clone(), nd[2], lengths, nl)
    assert torch.equal(bits(room), bits(by_hand))


def test_random_crops_reproduce_themselves_and_draw_as_before_without_pitch(corpus):
    import torch

    import alac.net_amd as pkg

    spec = pkg.PitchShift(semitones=(-3, 0, 3), p=0.8, n_fft=1024)
    gen = lambda: torch.Generator(device="cuda").manual_seed(2)
    a = corpus.random_crops(6, L, generator=gen(), pitch=spec)
    b = corpus.random_crops(6, L, generator=gen(), pitch=spec)
    assert all(torch.equal(s, t) for s, t in zip(a[1:], b[1:])) and torch.equal(bits(a[0]), bits(b[0]))
    # the draw sits behind the call's own two: files and offsets are those of the call without pitch=
    g1, g2 = gen(), gen()
    plain = corpus.random_crops(6, L, generator=g1)
    assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and torch.equal(plain[1], a[1])
    draws = spec.draw(6, generator=g1)
    corpus.random_crops(6, L, generator=g2, pitch=spec)
    assert torch.equal(g1.get_state(), g2.get_state())
    want = pkg.pitch_shift(plain[0].clone(), [spec.ratios[k] for k in draws.tolist()], RATE, plain[1], 1024)
    assert torch.equal(bits(a[0]), bits(want)) and not torch.equal(bits(a[0]), bits(plain[0]))
    # without pitch= the generator is consumed exactly as before: a noise mix draws what it drew
    add = pkg.AddNoise(corpus, (5.0, 15.0))
    g3, g4 = gen(), gen()
    corpus.random_crops(6, L, generator=g3, mix=add)
    corpus.random_crops(6, L, generator=g4, mix=add, pitch=None)
    assert torch.equal(g3.get_state(), g4.get_state())
    feats = corpus.random_crops(6, L, generator=gen(), pitch=spec, features=pkg.KaldiFbank(RATE), mono=True)
    assert feats[0].shape[:3] == (6, 1, 80) and bool(torch.isfinite(feats[0]).all()) and torch.equal(feats[2], plain[2])


def test_the_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    spec, draws = policy(pkg, torch)
    for kw in (dict(pitch="up"), dict(pitch=1.1), dict(pitch=pkg.SpeedPerturb()), dict(pitch=spec, dtype=torch.int32),
               dict(pitch=(spec, draws[:3])), dict(pitch=(spec, draws.float())), dict(pitch=(spec, draws.cpu())),
               dict(pitch=(spec, draws.view(2, 3))), dict(pitch=(spec, draws.tolist()))):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, check=False, **kw)
    for kw in (dict(pitch="up"), dict(pitch=spec, dtype=torch.int32), dict(pitch=(spec, draws[:3]))):
        with pytest.raises(ValueError):
            corpus.random_crops(6, L, **kw)
    with pytest.raises(ValueError):
        corpus.crops(cf, co, 256, check=False, pitch=spec)           # num_frames <= n_fft // 2
    with pytest.raises(ValueError):
        corpus.random_crops(4, 1024, pitch=pkg.PitchShift(n_fft=2048))
    # a call without pitch= returns the bits it returned
    first = [t.clone() for t in corpus.crops(cf, co, L, check=False)]
    corpus.crops(cf, co, L, check=False, pitch=(spec, draws))
    again = corpus.crops(cf, co, L, check=False)
    assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(first[1], again[1])


def test_crops_without_a_rate_are_refused(tmp_path):
    import torch

    import alac.net_amd as pkg

    paths = []
    for i, rate in enumerate((16000, 22050)):
        x = torch.from_numpy((0.1 * np.random.default_rng(i).standard_normal((1, 4000))).astype(np.float32)).cuda()
        paths.append(str(tmp_path / f"m{i}.m4a"))
        pkg.save(paths[-1], x, rate, sample_size=16, frame_length=1024)
    with pkg.Corpus(paths, mixed_rates=True) as c:
        cf, co = torch.tensor([0, 1], device="cuda"), torch.tensor([0, 10], device="cuda")
        with pytest.raises(ValueError):
            c.crops(cf, co, 2000, check=False, pitch=pkg.PitchShift())
        got, lengths = c.crops(cf, co, 2000, check=False, sample_rate=8000, pitch=(pkg.PitchShift(), torch.tensor([0, 4], device="cuda")))
        pcm = c.crops(cf, co, 2000, check=False, sample_rate=8000)[0].clone()
        want = pkg.pitch_shift(pcm, [pkg.PitchShift().ratios[0], pkg.PitchShift().ratios[4]], 8000, lengths)
        assert torch.equal(bits(got), bits(want))
