"""Corpus.crops(level=) and Corpus.random_crops(level=) on the GPU, on a synthetic corpus of four short files written with `save`
at three levels 30 dB apart: the stage's place in a step.  What the kernel computes is tests/test_level.py's subject; here crops
with level= are held bit for bit to alac.level of the crops without it -- natively, with sample_rate= and mono=, from a corpus
of mixed rates, behind reverb= and mix= and in front of effects= and a KaldiFbank --, a crop outside the corpus to zeros, the
generator to the draws it made without level=, and the refusals to ValueError before any device work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 8000          # four hops of 1600 frames and a few more: the least a loudness needs at 16 kHz
RATE = 16000
FILES = [(20000, 16, 4096, 1, 0.3), (9001, 24, 1024, 2, 0.01), (15000, 16, 1024, 3, 0.1), (7000, 16, 4096, 4, 0.03)]


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def write(pkg, torch, d, rate, tag, files=FILES):
    paths = []
    for i, (frames, size, fl, seed, amp) in enumerate(files):
        rng = np.random.default_rng(seed)
        t = np.arange(frames) / rate
        x = np.stack([amp * np.sin(2 * np.pi * (200.0 + 150 * seed) * t + c) + 0.1 * amp * rng.standard_normal(frames) for c in (0, 1)])
        paths.append(str(d / f"{tag}{i}.m4a"))
        pkg.save(paths[-1], torch.from_numpy(x.astype(np.float32)).cuda(), rate, sample_size=size, frame_length=fl)
    return paths


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(write(pkg, torch, tmp_path_factory.mktemp("corpus_level"), RATE, "lv")) as c:
        yield c


def device_crops(torch, corpus, sample_rate=None):
    """A start, a middle, one that runs off its file's end, another start, and the last outside the corpus"""
    totals = corpus.num_frames if sample_rate is None else corpus.resampled_frames(sample_rate)
    cf = [0, 1, 2, 3, corpus.num_files]
    co = [0, 1000, int(totals[2]) - L // 2, 17, 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


def specs(pkg):
    return [pkg.Level.lufs(-23.0, max_peak=0.99), pkg.Level.rms(-25.0, clamp=True), pkg.Level.peak(0.5)]


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=8000, mono=True)], ids=["native", "resampled-mono"])
def test_crops_with_level_are_level_of_the_crops(corpus, kw):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus, kw.get("sample_rate"))
    rate = kw.get("sample_rate", RATE)
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    for spec in specs(pkg):
        want = pkg.level(pcm, spec, rate, lengths)
        got, glen = corpus.crops(cf, co, L, check=False, level=spec, **kw)
        assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(want)), spec
        assert lengths.tolist()[-1] == -1 and bool((got[-1] == 0).all()) and 0 < lengths.tolist()[2] < L
        assert not torch.equal(bits(got[0]), bits(pcm[0]))
    # the crops reach one loudness from files 30 dB apart
    got = corpus.crops(cf, co, L, check=False, level=pkg.Level.lufs(-23.0), **kw)
    loud = pkg.loudness(got[0], rate, got[1])
    whole = got[1] >= 4 * (rate // 10)                # (a crop shorter than a block, or outside the corpus, is not measured)
    assert whole.tolist()[:2] == [True, True] and not whole.tolist()[4]
    assert float((loud[whole] - -23.0).abs().max()) < 1e-3 and bool((loud[~whole] == float("-inf")).all()), loud
    # behind it the features see the levelled waveform; host indices give the same crops
    spec, feat = pkg.Level.rms(-25.0), pkg.KaldiFbank(rate, n_mels=23)
    feats, flen = corpus.crops(cf, co, L, check=False, level=spec, features=feat, normalize=pkg.MeanVar(), **kw)
    by_hand = pkg.normalize(pkg.fbank(pkg.level(pcm, spec, rate, lengths), feat), pkg.MeanVar(), flen)
    assert torch.equal(bits(feats), bits(by_hand))
    host = corpus.crops(cf[:4].tolist(), co[:4].tolist(), L, level=spec, **kw)
    assert torch.equal(bits(host[0]), bits(pkg.level(pcm, spec, rate, lengths)[:4]))


def test_the_order_is_reverb_mix_level_effects(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    add, rev = pkg.AddNoise(corpus, (5.0, 15.0)), pkg.Reverb(corpus, max_seconds=0.02)
    fx = pkg.Effects((pkg.RandomBiquad("highpass", (40.0, 120.0)),), gain=(0.125, 2.0))
    g = torch.Generator(device="cuda").manual_seed(3)
    front = dict(mix=(add, add.draw(5, L, generator=g)), reverb=(rev, rev.draw(5, generator=g)))
    draws = fx.draw(5, RATE, generator=g)
    spec = pkg.Level.lufs(-26.0)
    pcm, lengths = corpus.crops(cf, co, L, check=False, **front)
    levelled = pkg.level(pcm.clone(), spec, RATE, lengths)
    want = pkg.biquad(levelled, draws[0], lengths, draws[1])
    got, _ = corpus.crops(cf, co, L, check=False, level=spec, effects=(fx, draws), **front)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(corpus.crops(cf, co, L, check=False, level=spec, **front)[0]), bits(levelled))
    # ... so the random gain perturbs around the target: the loudness is the target plus the gain's decibels
    flat = pkg.Effects(gain=(0.125, 2.0))
    d2 = flat.draw(5, RATE, generator=g)
    out, olen = corpus.crops(cf, co, L, check=False, level=spec, effects=(flat, d2))
    moved = pkg.loudness(out, RATE, olen) - (-26.0 + 20.0 * torch.log10(d2[1]))
    assert float(moved[[0, 1, 3]].abs().max()) < 1e-3, moved


def test_a_corpus_of_mixed_rates(tmp_path):
    import torch

    import alac.net_amd as pkg

    paths = write(pkg, torch, tmp_path, RATE, "a")[:2] + write(pkg, torch, tmp_path, 22050, "b")[2:]
    with pkg.Corpus(paths, mixed_rates=True) as c:
        cf, co = torch.tensor([0, 1, 2, 3], device="cuda"), torch.tensor([0, 100, 50, 17], device="cuda")
        pcm, lengths = c.crops(cf, co, L, check=False, sample_rate=8000)
        pcm = pcm.clone()
        spec = pkg.Level.lufs(-23.0)
        got, _ = c.crops(cf, co, L, check=False, sample_rate=8000, level=spec)
        assert torch.equal(bits(got), bits(pkg.level(pcm, spec, 8000, lengths)))
        with pytest.raises(ValueError):
            c.crops(cf, co, L, check=False, level=spec)              # no rate of its own


def test_a_corpus_at_44100_hz_a_hop_longer_than_a_tile(tmp_path):
    """The rate of the project's own material: hops of 4410 frames, longer than the measure launch's tile of 4096, so a hop's sum
    is carried from tile to tile; crops of six hops and 37 frames, one that runs off its file's end and one outside the corpus"""
    import torch

    import alac.net_amd as pkg

    rate, n = 44100, 6 * 4410 + 37
    files = [(40000, 16, 4096, 1, 0.3), (30011, 24, 1024, 2, 0.01), (36000, 16, 4096, 3, 0.1)]
    with pkg.Corpus(write(pkg, torch, tmp_path, rate, "cd", files)) as c:
        cf, co = torch.tensor([0, 1, 2, c.num_files], device="cuda"), torch.tensor([0, 1000, 36000 - 5 * 4410, 0], device="cuda")
        pcm, lengths = c.crops(cf, co, n, check=False)
        pcm = pcm.clone()
        assert lengths.tolist() == [n, n, 5 * 4410, -1]
        for spec in (pkg.Level.lufs(), pkg.Level.lufs(-16.0, max_peak=0.5, clamp=True)):
            want = pkg.level(pcm, spec, rate, lengths)
            got, glen = c.crops(cf, co, n, check=False, level=spec)
            assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(want)), spec
            assert bool((got[-1] == 0).all()) and all(not torch.equal(bits(got[b]), bits(pcm[b])) for b in range(3))
        got, glen = c.crops(cf, co, n, check=False, level=pkg.Level.lufs())
        loud = pkg.loudness(got, rate, glen)
        assert float((loud[:3] - -23.0).abs().max()) < 1e-3 and float(loud[3]) == float("-inf"), loud


def test_random_crops_draw_what_they_drew_without_level(corpus):
    import torch

    import alac.net_amd as pkg

    spec = pkg.Level.lufs(-23.0)
    gen = lambda: torch.Generator(device="cuda").manual_seed(2)
    g1, g2 = gen(), gen()
    plain = corpus.random_crops(6, L, generator=g1)
    a = corpus.random_crops(6, L, generator=g2, level=spec)
    assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and torch.equal(plain[1], a[1])
    assert torch.equal(g1.get_state(), g2.get_state())              # it draws nothing
    assert torch.equal(bits(a[0]), bits(pkg.level(plain[0].clone(), spec, RATE, plain[1])))
    feats = corpus.random_crops(6, L, generator=gen(), level=spec, effects=pkg.Effects(gain=(0.5, 2.0)), features=pkg.KaldiFbank(RATE), mono=True)
    assert feats[0].shape[:3] == (6, 1, 80) and bool(torch.isfinite(feats[0]).all()) and torch.equal(feats[2], plain[2])


def test_the_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    cf, co = device_crops(torch, corpus)
    for kw in (dict(level="lufs"), dict(level=-23.0), dict(level=(pkg.Level.lufs(), None)), dict(level=pkg.Level.lufs(), dtype=torch.int32),
               dict(level=pkg.Level.peak(), dtype=torch.int32), dict(level=pkg.Level.lufs(), sample_rate=150),
               dict(level=pkg.Level.lufs(), sample_rate=2000)):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, check=False, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(4, L, **kw)
    with pytest.raises(ValueError):
        pkg.Level.lufs(float("inf"))
    # a call without level= returns the bits it returned
    first = [t.clone() for t in corpus.crops(cf, co, L, check=False)]
    corpus.crops(cf, co, L, check=False, level=pkg.Level.peak(0.25))
    again = corpus.crops(cf, co, L, check=False)
    assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(first[1], again[1])
