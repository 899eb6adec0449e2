"""Corpus.crops(reverb=) and Corpus.random_crops(reverb=) on the GPU: the stage's place in a step.  What the kernel computes
is tests/test_reverb.py's subject; here crops with reverb= are held bit for bit to alac.reverb of the crops without it and
the responses the corpus of impulse responses makes, on the native path, on the sample_rate= / mono= path, in front of mix=,
features= and normalize=; p = 0 to the crops themselves; the draws to a seed; check=False to no read-back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
RATE = 44100
SECONDS = 0.05                    # 2205 frames at 44.1 kHz (two partitions), 800 at 16 kHz


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpora(synth, tmp_path_factory):
    """The signal (three stereo files), a noise corpus, and two corpora of impulse responses written with `save`:
    exponentially decaying noise of 300 .. 6000 frames, one channel at 44.1 and 16 kHz (mixed_rates=True), and two channels"""
    import torch

    import alac.net_amd as pkg
    from test_load_window import make_file

    sig = [make_file(synth, n, last, ss, True, seed=160 + i)[0] for i, (n, last, ss) in enumerate([(3, 100, 16), (2, 4000, 24), (4, 1234, 16)])]
    noise = [make_file(synth, n, last, 16, False, seed=180 + i)[0] for i, (n, last) in enumerate([(2, 2000), (1, 700)])]
    d = tmp_path_factory.mktemp("rirs")
    rng = np.random.default_rng(7)

    def response(channels, frames, rate, name):
        h = 0.3 * rng.standard_normal((channels, frames)) * np.exp(-np.arange(frames) / (frames / 6.0))
        h[:, 10 + 3 * np.arange(channels)] = 0.9                                  # the direct path, later in the second channel
        path = str(d / name)
        pkg.save(path, torch.from_numpy(h.astype(np.float32)).cuda(), rate, frame_length=1024)
        return path

    mono = [response(1, frames, rate, f"m{i}.m4a") for i, (frames, rate) in enumerate([(300, 44100), (6000, 44100), (1500, 16000), (4000, 16000)])]
    stereo = [response(2, frames, 44100, f"s{i}.m4a") for i, frames in enumerate([500, 5000])]
    with pkg.Corpus(sig) as c, pkg.Corpus(noise) as n, pkg.Corpus(mono, mixed_rates=True) as rm, pkg.Corpus(stereo) as rs:
        assert (c.channels, rm.channels, rs.channels) == (2, 1, 2) and rm.sample_rate is None
        yield dict(sig=c, noise=n, mono=rm, stereo=rs, sig_files=sig)


def device_crops(torch, corpus, totals):
    """A start, a middle, one that runs off its file's end, another middle, and the last outside the corpus"""
    cf = [0, 1, 2, 2, 1, corpus.num_files]
    co = [0, int(totals[1]) // 3, max(int(totals[2]) - L // 2, 0), 17, 100, 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


def by_hand(pkg, corpus, aug, cf, co, draws, **kw):
    """alac.reverb of the crops without reverb= and the responses: (reverberated, lengths, crops, responses, their lengths)"""
    import torch

    rf, keep = draws
    rirs = aug.rirs
    rate = kw.get("sample_rate") or corpus.sample_rate
    Co = 1 if kw.get("mono") else corpus.channels
    K = aug.frames(rate)
    h, hlen = rirs.crops(rf, torch.zeros_like(rf), K, sample_rate=rate, mono=rirs.channels != Co, check=False)
    h = h.clone()
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    return pkg.reverb(pcm, h, lengths, torch.where(keep, hlen, 0)), lengths, pcm, h, hlen


@pytest.mark.parametrize("which", ["stereo", "mono"])
def test_native_crops_with_reverb_are_reverb_of_the_crops(corpora, which):
    import torch

    import alac.net_amd as pkg

    corpus, rirs = corpora["sig"], corpora[which]
    cf, co = device_crops(torch, corpus, corpus.num_frames)
    aug = pkg.Reverb(rirs, p=0.7, max_seconds=SECONDS)
    files, keep = aug.draw(64, generator=torch.Generator(device="cuda").manual_seed(1))
    assert bool(((files >= 0) & (files < rirs.num_files)).all()) and 24 <= int(keep.sum()) <= 60          # p = 0.7 of 64
    n = rirs.num_files
    draws = (torch.tensor([0, 1, n - 1, 1, 0, 1], device="cuda"), torch.tensor([True, False, True, True, True, True], device="cuda"))
    want, wlen, pcm, h, hlen = by_hand(pkg, corpus, aug, cf, co, draws)
    K = aug.frames(RATE)
    assert h.shape == (6, 2 if which == "stereo" else 1, K) and K == 2205 and (hlen.cpu() < K).any() and (hlen.cpu() == K).any()
    got, lengths = corpus.crops(cf, co, L, reverb=(aug, draws), check=False)
    st = corpus.last_status()[0].clone()
    assert got.shape == (6, 2, L) and torch.equal(lengths, wlen) and torch.equal(bits(got), bits(want))
    assert lengths.tolist()[-1] == -1 and 0 < lengths.tolist()[2] < L
    changed = draws[1] & (lengths > 0)
    for b in range(6):
        assert torch.equal(bits(got[b]), bits(pcm[b])) != bool(changed[b]), b
        assert torch.equal(got[b, :, max(int(lengths[b]), 0):], pcm[b, :, max(int(lengths[b]), 0):])
    corpus.crops(cf, co, L, check=False)
    assert torch.equal(corpus.last_status()[0], st)                                              # last_status() is the crops' own
    out = torch.full_like(got, 3.0)
    assert corpus.crops(cf, co, L, reverb=(aug, draws), check=False, out=out)[0] is out and torch.equal(bits(out), bits(got))
    with pytest.raises(ValueError):
        corpus.crops(cf, co, L, reverb=(aug, draws))                                             # check=True names the crop outside
    host = corpus.crops(cf[:5].tolist(), co[:5].tolist(), L, reverb=(aug, tuple(t[:5] for t in draws)))
    assert torch.equal(bits(host[0]), bits(got[:5]))
    # a Reverb alone is drawn from the device's default generator
    torch.cuda.manual_seed(11)
    a, _ = corpus.crops(cf, co, L, reverb=aug, check=False)
    torch.cuda.manual_seed(11)
    d2 = aug.draw(len(cf))
    assert torch.equal(bits(a), bits(corpus.crops(cf, co, L, reverb=(aug, d2), check=False)[0]))


def test_resampled_mono_crops_with_responses_of_other_rates(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    cf, co = device_crops(torch, corpus, corpus.resampled_frames(16000))
    for which in ("mono", "stereo"):
        aug = pkg.Reverb(corpora[which], max_seconds=SECONDS)
        draws = aug.draw(len(cf), generator=torch.Generator().manual_seed(2))                    # a CPU generator
        for kw in (dict(sample_rate=16000, mono=True), dict(sample_rate=16000, mono=False)):
            want, wlen, pcm, h, hlen = by_hand(pkg, corpus, aug, cf, co, draws, **kw)
            Co = 1 if kw["mono"] else 2
            assert h.shape == (6, Co if which == "stereo" and Co == 2 else 1, 800) and pcm.shape == (6, Co, L)
            got, lengths = corpus.crops(cf, co, L, reverb=(aug, draws), check=False, **kw)
            assert torch.equal(lengths, wlen) and torch.equal(bits(got), bits(want)) and not torch.equal(got[0], pcm[0]), (which, kw)


def test_mix_features_and_normalize_follow_the_reverberated_waveform(corpora):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.features import feature_lengths

    corpus, noise = corpora["sig"], corpora["noise"]
    kw = dict(sample_rate=16000, mono=True)
    spec = pkg.LogMel(16000, 400, 160, 80, log="log10")
    cf, co = device_crops(torch, corpus, corpus.resampled_frames(16000))
    aug, add = pkg.Reverb(corpora["mono"], p=0.8, max_seconds=SECONDS), pkg.AddNoise(noise, (0, 15))
    g = torch.Generator(device="cuda").manual_seed(3)
    draws, ndraws = aug.draw(len(cf), generator=g), add.draw(len(cf), L, sample_rate=16000, generator=g)
    wave, lengths = corpus.crops(cf, co, L, reverb=(aug, draws), check=False, **kw)
    wave = wave.clone()
    assert torch.equal(bits(wave), bits(by_hand(pkg, corpus, aug, cf, co, draws, **kw)[0]))
    # the noise goes onto the reverberated crop
    ncrops, nlen = noise.crops(ndraws[0], ndraws[1], L, sample_rate=16000, check=False)
    mixed_want = pkg.mix(wave, ncrops.clone(), ndraws[2], lengths, nlen)
    mixed, mlen = corpus.crops(cf, co, L, reverb=(aug, draws), mix=(add, ndraws), check=False, **kw)
    mixed = mixed.clone()
    assert torch.equal(mlen, lengths) and torch.equal(bits(mixed), bits(mixed_want)) and not torch.equal(mixed, wave)
    feats, flen = corpus.crops(cf, co, L, reverb=(aug, draws), mix=(add, ndraws), features=spec, check=False, **kw)
    feats = feats.clone()
    assert torch.equal(bits(feats), bits(pkg.log_mel(mixed, spec))) and torch.equal(flen, feature_lengths(lengths, 160))
    plain, _ = corpus.crops(cf, co, L, reverb=(aug, draws), features=spec, check=False, **kw)
    assert torch.equal(bits(plain), bits(pkg.log_mel(wave, spec))) and not torch.equal(plain, feats)
    for how in (pkg.TopDb.whisper(), pkg.MeanVar()):
        got, glen = corpus.crops(cf, co, L, reverb=(aug, draws), mix=(add, ndraws), features=spec, normalize=how, check=False, **kw)
        assert torch.equal(glen, flen) and torch.equal(bits(got), bits(pkg.normalize(feats, how, flen))), how
    got, glen = corpus.crops(cf, co, L, reverb=(aug, draws), normalize=pkg.MeanVar(), check=False, **kw)
    assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(pkg.normalize(wave, pkg.MeanVar(), lengths)))


def test_random_crops_are_reproducible_and_p_0_is_no_reverberation(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    aug = pkg.Reverb(corpora["stereo"], p=0.9, max_seconds=SECONDS)
    for dev in ("cuda", "cpu"):
        a = corpus.random_crops(8, L, generator=torch.Generator(device=dev).manual_seed(5), reverb=aug)
        b = corpus.random_crops(8, L, generator=torch.Generator(device=dev).manual_seed(5), reverb=aug)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), dev
        # the call's own two draws, then Reverb.draw's two, from one generator
        g = torch.Generator(device=dev).manual_seed(5)
        plain = corpus.random_crops(8, L, generator=g)
        draws = aug.draw(8, generator=g)
        assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and torch.equal(plain[1], a[1])
        again = corpus.crops(a[2], a[3], L, reverb=(aug, draws))
        assert torch.equal(bits(again[0]), bits(a[0])) and not torch.equal(a[0], plain[0]), dev
    none = pkg.Reverb(corpora["stereo"], p=0.0, max_seconds=SECONDS)
    a = corpus.random_crops(8, L, generator=torch.Generator(device="cuda").manual_seed(6), reverb=none)
    assert torch.equal(bits(a[0]), bits(corpus.crops(a[2], a[3], L)[0]))
    cf, co = device_crops(torch, corpus, corpus.num_frames)
    assert torch.equal(bits(corpus.crops(cf, co, L, reverb=none, check=False)[0]), bits(corpus.crops(cf, co, L, check=False)[0].clone()))
    both = corpus.random_crops(4, L, generator=torch.Generator().manual_seed(7), reverb=aug, mix=pkg.AddNoise(corpora["noise"], 10.0),
                               features=pkg.LogMel(RATE, 400, 160, 80))
    assert both[0].shape == (4, 2, 80, 1 + L // 160)


def test_check_false_reads_nothing_back(corpora):
    # torch's sync debug mode raises on every synchronising call torch itself makes: in "error" mode the whole step runs through
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    spec = pkg.LogMel(16000, 400, 160, 80)
    for rirs, kw in ((corpora["stereo"], {}), (corpora["mono"], dict(sample_rate=16000, mono=True, features=spec))):
        aug = pkg.Reverb(rirs, p=0.8, max_seconds=SECONDS)
        totals = corpus.num_frames if not kw else corpus.resampled_frames(16000)
        cf, co = device_crops(torch, corpus, totals)
        g = torch.Generator(device="cuda").manual_seed(10)
        draws = aug.draw(len(cf), generator=g)
        want, want_len = corpus.crops(cf, co, L, reverb=(aug, draws), check=False, **kw)       # (also the first call's allocations)
        want = want.clone()
        corpus.random_crops(4, L, generator=g, reverb=aug, check=False, **kw)
        out = torch.empty_like(want)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                want_len.cpu()
            got, lengths = corpus.crops(cf, co, L, reverb=(aug, draws), check=False, **kw)
            got2, _ = corpus.crops(cf, co, L, reverb=(aug, draws), check=False, out=out, **kw)
            drawn, _ = corpus.crops(cf, co, L, reverb=aug, check=False, **kw)
            r = corpus.random_crops(4, L, generator=g, reverb=aug, check=False, **kw)
            with pytest.raises(RuntimeError):
                corpus.crops(cf, co, L, reverb=(aug, draws), check=True, **kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(bits(got), bits(want)) and got2 is out and torch.equal(bits(out), bits(want)) and torch.equal(lengths, want_len)
        assert drawn.shape == want.shape and r[0].shape[0] == 4


def test_what_cannot_be_reverberated_is_refused_before_any_device_work(corpora):
    import torch

    import alac.net_amd as pkg

    corpus, rirs = corpora["sig"], corpora["stereo"]
    aug = pkg.Reverb(rirs, max_seconds=SECONDS)
    corpus.crops([0], [0], L)
    before = corpus.last_status()[0].clone()
    draws = aug.draw(1)
    with pkg.Corpus(corpora["sig_files"][:1]) as gone:
        closed = pkg.Reverb(gone)
    bad = [dict(reverb=aug, dtype=torch.int32), dict(reverb="room"), dict(reverb=rirs), dict(reverb=(aug,)), dict(reverb=(aug, draws[:1])),
           dict(reverb=(aug, (draws[0], draws[0]))), dict(reverb=(aug, (draws[0].float(), draws[1]))),
           dict(reverb=(aug, tuple(t.cpu() for t in draws))), dict(reverb=(aug, [1, 2])), dict(reverb=(draws, aug)), dict(reverb=closed),
           dict(reverb=(closed, draws))]
    for kw in bad:
        with pytest.raises(ValueError):
            corpus.crops([0], [0], L, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(1, L, **kw)
    with pytest.raises(ValueError):
        corpus.crops([0, 1], [0, 0], L, reverb=(aug, draws))                    # one draw for two crops
    # a corpus whose rates differ has no rate of its own for the crops, and so none for the responses
    rated = corpora["mono"]
    with pytest.raises(ValueError):
        rated.crops([0], [0], L, reverb=aug)
    with pytest.raises(ValueError):
        rated.random_crops(1, L, reverb=aug)
    if torch.cuda.device_count() > 1:
        with pkg.Corpus(corpora["sig_files"][:1], device=1) as far:
            with pytest.raises(ValueError):
                corpus.crops([0], [0], L, reverb=pkg.Reverb(far))
    assert torch.equal(corpus.last_status()[0], before)                          # nothing ran
    assert rated.crops([0], [0], L, sample_rate=16000, reverb=pkg.Reverb(corpus, max_seconds=SECONDS))[0].shape == (1, 1, L)
