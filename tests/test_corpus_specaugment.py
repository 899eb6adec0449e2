"""Corpus.crops(augment=) and Corpus.random_crops(augment=) on the GPU: the stage's place in a step.  What the kernel computes
is tests/test_specaugment.py's subject; here crops with augment= are held bit for bit to alac.spec_augment of what the call
returns without it, with and without normalize=, on a corpus of one rate and on one whose rates differ; the draws to a seed;
a crop outside the corpus to being left alone; check=False to no read-back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 6000
RATE = 44100


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpora(synth, tmp_path_factory):
    """Three short stereo files of one rate, and three mono files of two rates"""
    import torch

    import alac.net_amd as pkg
    from test_load_window import make_file

    sig = [make_file(synth, n, last, ss, True, seed=160 + i)[0] for i, (n, last, ss) in enumerate([(3, 100, 16), (2, 4000, 24), (4, 1234, 16)])]
    d = tmp_path_factory.mktemp("augment_rated")
    rated = []
    for i, (rate, frames) in enumerate([(16000, 9000), (22050, 12000), (16000, 3000)]):
        t = np.arange(frames) / rate
        x = 0.3 * np.sin(2 * np.pi * 200 * (i + 1) * t) + 0.05 * np.random.default_rng(190 + i).standard_normal(frames)
        path = str(d / f"a{i}_{rate}.m4a")
        pkg.save(path, torch.from_numpy(x[None].astype(np.float32)).cuda(), rate, frame_length=1024)
        rated.append(path)
    with pkg.Corpus(sig) as c, pkg.Corpus(rated, mixed_rates=True) as r:
        assert c.channels == 2 and r.sample_rate is None
        yield dict(sig=c, rated=r)


def device_crops(torch, corpus, totals):
    """A start, a middle, one that runs off its file's end, and the last outside the corpus"""
    cf = [0, 1, 2, corpus.num_files]
    co = [0, int(totals[1]) // 3, max(int(totals[2]) - L // 2, 0), 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


@pytest.mark.parametrize("which", ["sig", "rated"])
def test_crops_with_augment_are_spec_augment_of_the_crops_without(corpora, which):
    import torch

    import alac.net_amd as pkg

    corpus = corpora[which]
    kw = dict(sample_rate=16000, mono=True) if which == "rated" else {}
    rate = kw.get("sample_rate", RATE)
    totals = corpus.resampled_frames(16000) if which == "rated" else corpus.num_frames
    cf, co = device_crops(torch, corpus, totals)
    spec = pkg.LogMel(rate, 400, 160, 80, log="log10")
    aug = pkg.SpecAugment(freq_masks=2, freq_width=27, time_masks=2, time_width=10, time_warp=3, fill=-0.5)
    for how in (None, pkg.MeanVar(), pkg.TopDb.whisper()):
        plain, flen = corpus.crops(cf, co, L, features=spec, normalize=how, check=False, **kw)
        plain = plain.clone()
        draws = aug.draw(80, flen, generator=torch.Generator(device="cuda").manual_seed(21))
        want = pkg.spec_augment(plain, (aug, draws), flen)
        got, glen = corpus.crops(cf, co, L, features=spec, normalize=how, augment=(aug, draws), check=False, **kw)
        assert got.shape == plain.shape and torch.equal(glen, flen) and torch.equal(bits(got), bits(want)), how
        f = flen.tolist()
        assert f[-1] == -1 and torch.equal(bits(got[-1]), bits(plain[-1]))           # a crop outside the corpus is left alone
        assert 0 < f[2] < plain.shape[3] and torch.equal(bits(got[2, ..., f[2]:]), bits(plain[2, ..., f[2]:]))
        assert all(not torch.equal(got[b], plain[b]) for b in range(3))
        out = torch.full_like(got, 3.0)
        assert corpus.crops(cf, co, L, features=spec, normalize=how, augment=(aug, draws), check=False, out=out, **kw)[0] is out
        assert torch.equal(bits(out), bits(got))
    # a SpecAugment alone is drawn from the device's default generator, for the feat_lengths of the call
    torch.cuda.manual_seed(22)
    a, _ = corpus.crops(cf, co, L, features=spec, augment=aug, check=False, **kw)
    a = a.clone()
    torch.cuda.manual_seed(22)
    d2 = aug.draw(80, flen.clamp(max=plain.shape[3]))
    assert torch.equal(bits(a), bits(corpus.crops(cf, co, L, features=spec, augment=(aug, d2), check=False, **kw)[0]))
    # check=True still names the crop outside the corpus
    with pytest.raises(ValueError):
        corpus.crops(cf, co, L, features=spec, augment=(aug, draws), **kw)


def test_random_crops_are_reproducible_and_draw_behind_the_earlier_draws(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    spec = pkg.LogMel(RATE, 400, 160, 80)
    aug = pkg.SpecAugment(time_width=8, time_warp=2, p=0.8)
    noise = pkg.AddNoise(corpus, (5, 20))
    for dev in ("cuda", "cpu"):
        a = corpus.random_crops(6, L, generator=torch.Generator(device=dev).manual_seed(25), features=spec, normalize=pkg.MeanVar(), augment=aug)
        b = corpus.random_crops(6, L, generator=torch.Generator(device=dev).manual_seed(25), features=spec, normalize=pkg.MeanVar(), augment=aug)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), dev
        # the call's own two draws, the noise's four, then SpecAugment.draw's, from one generator
        g = torch.Generator(device=dev).manual_seed(26)
        full = corpus.random_crops(6, L, generator=g, features=spec, mix=noise, augment=aug)
        g = torch.Generator(device=dev).manual_seed(26)
        plain = corpus.random_crops(6, L, generator=g, features=spec)
        nd = noise.draw(6, L, sample_rate=RATE, generator=g)
        draws = aug.draw(80, plain[1], generator=g)
        assert torch.equal(plain[2], full[2]) and torch.equal(plain[3], full[3]) and torch.equal(plain[1], full[1])
        again = corpus.crops(full[2], full[3], L, features=spec, mix=(noise, nd), augment=(aug, draws))
        assert torch.equal(bits(again[0]), bits(full[0])) and not torch.equal(full[0], plain[0]), dev
    none = corpus.random_crops(4, L, generator=torch.Generator().manual_seed(27), features=spec, augment=pkg.SpecAugment(p=0.0))
    assert torch.equal(bits(none[0]), bits(corpus.crops(none[2], none[3], L, features=spec)[0]))


def test_check_false_reads_nothing_back(corpora):
    # torch's sync debug mode raises on every synchronising call torch itself makes: in "error" mode the whole step runs through
    import torch

    import alac.net_amd as pkg

    for which, kw in (("sig", {}), ("rated", dict(sample_rate=16000, mono=True))):
        corpus = corpora[which]
        spec = pkg.LogMel(kw.get("sample_rate", RATE), 400, 160, 80)
        aug = pkg.SpecAugment(time_width=8, time_warp=2, p=0.8)
        cf, co = device_crops(torch, corpus, corpus.resampled_frames(16000) if kw else corpus.num_frames)
        g = torch.Generator(device="cuda").manual_seed(30)
        step = dict(features=spec, normalize=pkg.MeanVar(), check=False, **kw)
        flen = corpus.crops(cf, co, L, **step)[1]
        draws = aug.draw(80, flen, generator=g)
        want, want_len = corpus.crops(cf, co, L, augment=(aug, draws), **step)               # (also the first call's allocations)
        want = want.clone()
        corpus.random_crops(4, L, generator=g, augment=aug, **step)
        out = torch.empty_like(want)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                want_len.cpu()
            got, lengths = corpus.crops(cf, co, L, augment=(aug, draws), **step)
            got2, _ = corpus.crops(cf, co, L, augment=(aug, draws), out=out, **step)
            drawn, _ = corpus.crops(cf, co, L, augment=aug, **step)
            r = corpus.random_crops(4, L, generator=g, augment=aug, **step)
            again = aug.draw(80, flen, generator=g)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(bits(got), bits(want)) and got2 is out and torch.equal(bits(out), bits(want)) and torch.equal(lengths, want_len)
        assert drawn.shape == want.shape and r[0].shape[0] == 4 and again[0].shape == (4, 2)


def test_what_cannot_be_augmented_is_refused_before_any_device_work(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    spec = pkg.LogMel(RATE, 400, 160, 80)
    aug = pkg.SpecAugment(time_warp=2)
    corpus.crops([0], [0], L)
    before = corpus.last_status()[0].clone()
    draws = aug.draw(80, torch.tensor([38], device="cuda"))
    bad = [dict(augment=aug), dict(augment=(aug, draws)), dict(augment=aug, normalize=pkg.MeanVar()),              # no features=
           dict(features=spec, augment="spec"), dict(features=spec, augment=draws), dict(features=spec, augment=(aug,)),
           dict(features=spec, augment=(aug, draws[:2])), dict(features=spec, augment=(draws, aug)), dict(features=spec, augment=(aug, None)),
           dict(features=spec, augment=(aug, tuple(t.cpu() for t in draws))),
           dict(features=spec, augment=(aug, (draws[0], draws[1], draws[2].long()))),
           dict(features=spec, augment=(aug, (draws[0].reshape(2, 1), draws[1], draws[2])))]
    for kw in bad:
        with pytest.raises(ValueError):
            corpus.crops([0], [0], L, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(1, L, **kw)
    with pytest.raises(ValueError):
        corpus.crops([0, 1], [0, 0], L, features=spec, augment=(aug, draws))                     # one draw for two crops
    with pytest.raises(ValueError):
        corpus.crops([0], [0], 40 * 16385, features=pkg.LogMel(RATE, 64, 40, 8), augment=aug)   # 16385 feature frames: no warp
    assert torch.equal(corpus.last_status()[0], before)                                          # nothing ran
    assert corpus.crops([0], [0], L, features=spec, augment=(aug, draws))[0].shape == (1, 2, 80, 38)
