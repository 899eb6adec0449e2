"""Corpus.crops(effects=) and Corpus.random_crops(effects=) on the GPU, on a synthetic corpus of four short files written with
`save`: the stage's place in a step.  What the kernel computes is tests/test_biquad.py's subject; here crops with effects= are
held bit for bit to alac.biquad of the crops without it -- natively, with sample_rate= and mono=, behind mix= and reverb=, in
front of a KaldiFbank and a MeanVar --, the draws to a seed, a crop outside the corpus to zeros, the refusals to ValueError
before any device work, and the call without effects= to the bits it returned before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 6000
RATE = 16000
FILES = [(20000, 16, 4096, 1), (9001, 24, 1024, 2), (15000, 16, 1024, 3), (7000, 16, 4096, 4)]


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    d = tmp_path_factory.mktemp("corpus_biquad")
    paths = []
    for i, (frames, size, fl, seed) in enumerate(FILES):
        rng = np.random.default_rng(seed)
        t = np.arange(frames) / RATE
        x = np.stack([0.3 * np.sin(2 * np.pi * (200.0 + 150 * seed) * t + c) + 0.05 * rng.standard_normal(frames) for c in (0, 1)])
        paths.append(str(d / f"fx{i}.m4a"))
        pkg.save(paths[-1], torch.from_numpy(x.astype(np.float32)).cuda(), RATE, sample_size=size, frame_length=fl)
    with pkg.Corpus(paths) as c:
        yield c


def device_crops(torch, corpus, sample_rate=None):
    """A start, a middle, one that runs off its file's end, another start, and the last outside the corpus; the offsets count
    frames at the rate of the crops"""
    totals = corpus.num_frames if sample_rate is None else corpus.resampled_frames(sample_rate)
    cf = [0, 1, 2, 3, corpus.num_files]
    co = [0, 1000, int(totals[2]) - L // 2, 17, 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


def policy(pkg):
    return pkg.Effects((pkg.RandomBiquad("highpass", (40.0, 120.0)), pkg.RandomBiquad("peaking", (300.0, 3000.0), q=(0.5, 2.0),
                                                                                     gain_db=(-8.0, 8.0), p=0.6),
                        pkg.RandomBiquad("lowpass", (2500.0, 3800.0), p=0.8)), gain=(0.125, 2.0), p=0.8, clamp=True)


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=8000, mono=True), dict(stages=True)], ids=["native", "resampled-mono", "mix-reverb"])
def test_crops_with_effects_are_biquad_of_the_crops(corpus, kw):
    import torch

    import alac.net_amd as pkg

    fx = policy(pkg)
    cf, co = device_crops(torch, corpus, kw.get("sample_rate"))
    if kw.pop("stages", False):
        add, rev = pkg.AddNoise(corpus, (5.0, 15.0)), pkg.Reverb(corpus, max_seconds=0.02)
        g = torch.Generator(device="cuda").manual_seed(3)
        kw = dict(mix=(add, add.draw(5, L, generator=g)), reverb=(rev, rev.draw(5, generator=g)))
    rate = kw.get("sample_rate", RATE)
    draws = fx.draw(5, rate, generator=torch.Generator(device="cuda").manual_seed(5))
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    want = pkg.biquad(pcm, draws[0], lengths, draws[1], clamp=True)
    got, glen = corpus.crops(cf, co, L, check=False, effects=(fx, draws), **kw)
    assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(want))
    assert lengths.tolist()[-1] == -1 and bool((got[-1] == 0).all()) and 0 < lengths.tolist()[2] < L
    assert not torch.equal(bits(got[0]), bits(pcm[0]))
    # behind it the features and the normalisation see the filtered waveform
    spec, how = pkg.KaldiFbank(rate, n_mels=23), pkg.MeanVar()
    feats, flen = corpus.crops(cf, co, L, check=False, effects=(fx, draws), features=spec, normalize=how, **kw)
    by_hand = pkg.normalize(pkg.fbank(want, spec), how, flen)
    assert torch.equal(bits(feats), bits(by_hand))
    # host indices, and an Effects alone is drawn from the device's default generator
    host = corpus.crops(cf[:4].tolist(), co[:4].tolist(), L, effects=(fx, tuple(t[:4] for t in draws)), **{k: (v[0], tuple(t[:4] for t in v[1])) if isinstance(v, tuple) else v for k, v in kw.items()})
    assert torch.equal(bits(host[0]), bits(got[:4]))
    if not kw:
        torch.cuda.manual_seed(11)
        a, _ = corpus.crops(cf, co, L, effects=fx, check=False)
        torch.cuda.manual_seed(11)
        d2 = fx.draw(5, RATE, device="cuda")
        assert torch.equal(bits(a), bits(corpus.crops(cf, co, L, effects=(fx, d2), check=False)[0]))


def test_random_crops_are_reproducible_from_a_seed(corpus):
    import torch

    import alac.net_amd as pkg

    fx = policy(pkg)
    a = corpus.random_crops(6, L, generator=torch.Generator(device="cuda").manual_seed(2), effects=fx)
    b = corpus.random_crops(6, L, generator=torch.Generator(device="cuda").manual_seed(2), effects=fx)
    assert all(torch.equal(s, t) for s, t in zip(a[1:], b[1:])) and torch.equal(bits(a[0]), bits(b[0]))
    # the draws are Effects.draw's behind the call's own two
    g = torch.Generator(device="cuda").manual_seed(2)
    torch.randint(0, corpus.num_files, (6,), generator=g, device="cuda", dtype=torch.int64)
    torch.rand(6, generator=g, device="cuda", dtype=torch.float64)
    draws = fx.draw(6, RATE, generator=g)
    want = corpus.crops(a[2], a[3], L, effects=(fx, draws))[0]
    assert torch.equal(bits(a[0]), bits(want))
    plain = corpus.random_crops(6, L, generator=torch.Generator(device="cuda").manual_seed(2))
    assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and not torch.equal(bits(plain[0]), bits(a[0]))
    feats = corpus.random_crops(6, L, generator=torch.Generator(device="cuda").manual_seed(2), effects=pkg.Effects.telephone(),
                                features=pkg.KaldiFbank(RATE), mono=True)
    assert feats[0].shape[:3] == (6, 1, 80) and bool(torch.isfinite(feats[0]).all())


def test_the_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    fx = policy(pkg)
    cf, co = device_crops(torch, corpus)
    q, g = fx.draw(5, RATE, device="cuda")
    for kw in (dict(effects="telephone"), dict(effects=fx, dtype=torch.int32),
               dict(effects=(fx, (q[:4], g[:4]))), dict(effects=(fx, (q[:, :2], g))), dict(effects=(fx, (q.float(), g))),
               dict(effects=(fx, (q, g.float()))), dict(effects=(fx, (q.cpu(), g.cpu()))), dict(effects=(fx, (q, g[:4]))),
               dict(effects=(fx, q)), dict(effects=fx, sample_rate=7000), dict(effects=(fx, (q, g)), sample_rate=7600)):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, check=False, **kw)
    with pytest.raises(ValueError):
        corpus.random_crops(4, L, effects=fx, sample_rate=7000)
    with pytest.raises(ValueError):
        corpus.random_crops(4, L, effects=fx, dtype=torch.int32)


def test_a_call_without_effects_returns_the_bits_it_returned(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    first = [t.clone() for t in corpus.crops(cf, co, L, check=False)]
    corpus.crops(cf, co, L, check=False, effects=pkg.Effects(gain=(0.5, 0.5)))
    again = corpus.crops(cf, co, L, check=False)
    assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(first[1], again[1])
    # nothing drawn is nothing done: an Effects of no filter and no gain leaves the crops as they are
    same = corpus.crops(cf, co, L, check=False, effects=pkg.Effects())
    assert torch.equal(bits(first[0]), bits(same[0]))
