"""Corpus.crops(mix=) and Corpus.random_crops(mix=) on the GPU: the stage's place in a step.  What the kernel computes is
tests/test_mix.py's subject; here crops with mix= are held bit for bit to alac.mix of the crops without it and the noise
crops the noise corpus makes, on the native path, on the sample_rate= / mono= path and in front of features= and normalize=;
the draws to a seed; the achieved signal-to-noise ratio to the requested one; check=False to no read-back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
RATE = 44100


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpora(synth, tmp_path_factory):
    """The signal (three stereo files) and three noise corpora: stereo with a file shorter than a crop, mono, and mono of two
    other rates"""
    import torch

    import alac.net_amd as pkg
    from test_load_window import make_file

    sig = [make_file(synth, n, last, ss, True, seed=60 + i)[0] for i, (n, last, ss) in enumerate([(3, 100, 16), (2, 4000, 24), (4, 1234, 16)])]
    stereo = [make_file(synth, n, last, 16, True, seed=70 + i)[0] for i, (n, last) in enumerate([(1, 1500), (2, 500)])]
    mono = [make_file(synth, n, last, 16, False, seed=80 + i)[0] for i, (n, last) in enumerate([(2, 2000), (1, 700)])]
    d = tmp_path_factory.mktemp("mix_noise")
    rated = []
    for i, (rate, frames) in enumerate([(16000, 5000), (22050, 9000)]):
        t = np.arange(frames) / rate
        x = 0.2 * np.sin(2 * np.pi * 300 * (i + 1) * t) + 0.05 * np.random.default_rng(90 + i).standard_normal(frames)
        path = str(d / f"n{i}_{rate}.m4a")
        pkg.save(path, torch.from_numpy(x[None].astype(np.float32)).cuda(), rate, frame_length=1024)
        rated.append(path)
    with pkg.Corpus(sig) as c, pkg.Corpus(stereo) as ns, pkg.Corpus(mono) as nm, pkg.Corpus(rated, mixed_rates=True) as nr:
        assert (c.channels, ns.channels, nm.channels, nr.channels) == (2, 2, 1, 1) and nr.sample_rate is None
        yield dict(sig=c, stereo=ns, mono=nm, rated=nr, sig_files=sig)


def device_crops(torch, corpus, totals):
    """A start, a middle, one that runs off its file's end, another middle, and the last outside the corpus"""
    cf = [0, 1, 2, 2, 1, corpus.num_files]
    co = [0, int(totals[1]) // 3, max(int(totals[2]) - L // 2, 0), 17, 100, 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


def by_hand(pkg, corpus, noise, cf, co, draws, **kw):
    """alac.mix of the crops without mix= and the noise crops: (mixed, lengths, crops, noise crops, noise lengths)"""
    nf, no, snr = draws
    rate = kw.get("sample_rate") or corpus.sample_rate
    Co = 1 if kw.get("mono") else corpus.channels
    ncrops, nlen = noise.crops(nf, no, L, sample_rate=rate, mono=noise.channels != Co, check=False)
    ncrops = ncrops.clone()
    pcm, lengths = corpus.crops(cf, co, L, check=False, **kw)
    pcm = pcm.clone()
    return pkg.mix(pcm, ncrops, snr, lengths, nlen), lengths, pcm, ncrops, nlen


@pytest.mark.parametrize("which", ["stereo", "mono"])
def test_native_crops_with_mix_are_mix_of_the_crops(corpora, which):
    import torch

    import alac.net_amd as pkg

    corpus, noise = corpora["sig"], corpora[which]
    cf, co = device_crops(torch, corpus, corpus.num_frames)
    aug = pkg.AddNoise(noise, (5, 20), p=0.7)
    drawn = aug.draw(64, L, generator=torch.Generator(device="cuda").manual_seed(1))
    nf, no, snr = drawn
    assert nf.dtype == no.dtype == torch.int64 and snr.dtype == torch.float32 and all(t.is_cuda and t.shape == (64,) for t in drawn)
    s, totals = snr.cpu().numpy(), torch.from_numpy(noise.num_frames).cuda()
    assert ((s[~np.isnan(s)] >= 5) & (s[~np.isnan(s)] <= 20)).all() and 24 <= int((~np.isnan(s)).sum()) <= 60      # p = 0.7 of 64
    assert bool(((nf >= 0) & (nf < noise.num_files) & (no >= 0) & (no <= (totals[nf] - L).clamp(min=0))).all())
    # draws by hand, as the tensors they are: both noise files, the second crop without noise, some noise shorter than a crop
    draws = (torch.tensor([0, 1, 0, 1, 0, 1], device="cuda"), torch.tensor([0, 100, 200, 0, 1000, 50], device="cuda"),
             torch.tensor([10.0, float("nan"), 5.0, 20.0, 0.0, 15.0], device="cuda"))
    nf, no, snr = draws
    want, wlen, pcm, ncrops, nlen = by_hand(pkg, corpus, noise, cf, co, draws)
    got, lengths = corpus.crops(cf, co, L, mix=(aug, draws), check=False)
    st = corpus.last_status()[0].clone()
    assert got.shape == (6, 2, L) and torch.equal(lengths, wlen) and torch.equal(bits(got), bits(want))
    assert lengths.tolist()[-1] == -1 and 0 < lengths.tolist()[2] < L
    mixed = ~torch.isnan(snr) & (lengths > 0)
    assert ncrops.shape[1] == (2 if which == "stereo" else 1) and (nlen.cpu() < L).any()          # some noise is repeated
    for b in range(6):
        assert torch.equal(bits(got[b]), bits(pcm[b])) != bool(mixed[b]), b
        assert torch.equal(got[b, :, max(int(lengths[b]), 0):], pcm[b, :, max(int(lengths[b]), 0):])
    corpus.crops(cf, co, L, check=False)
    assert torch.equal(corpus.last_status()[0], st)                                              # last_status() is the crops' own
    out = torch.full_like(got, 3.0)
    assert corpus.crops(cf, co, L, mix=(aug, draws), check=False, out=out)[0] is out and torch.equal(bits(out), bits(got))
    # check=True still names the crop outside the corpus; host indices go through the host's checks
    with pytest.raises(ValueError):
        corpus.crops(cf, co, L, mix=(aug, draws))
    host = corpus.crops(cf[:5].tolist(), co[:5].tolist(), L, mix=(aug, tuple(t[:5] for t in draws)))
    assert torch.equal(bits(host[0]), bits(got[:5]))
    # an AddNoise alone is drawn from the device's default generator
    torch.cuda.manual_seed(11)
    a, _ = corpus.crops(cf, co, L, mix=aug, check=False)
    torch.cuda.manual_seed(11)
    d2 = aug.draw(len(cf), L, sample_rate=RATE)
    assert torch.equal(bits(a), bits(corpus.crops(cf, co, L, mix=(aug, d2), check=False)[0]))


def test_resampled_stereo_crops_with_mono_noise_of_other_rates(corpora):
    import torch

    import alac.net_amd as pkg

    corpus, noise = corpora["sig"], corpora["rated"]
    kw = dict(sample_rate=16000, mono=False)
    cf, co = device_crops(torch, corpus, corpus.resampled_frames(16000))
    aug = pkg.AddNoise(noise, 10.0)
    with pytest.raises(ValueError):
        aug.draw(len(cf), L)                                          # mixed rates: no rate to draw the offsets at
    draws = aug.draw(len(cf), L, sample_rate=16000, generator=torch.Generator().manual_seed(2))       # a CPU generator
    want, wlen, pcm, ncrops, nlen = by_hand(pkg, corpus, noise, cf, co, draws, **kw)
    assert ncrops.shape == (6, 1, L) and pcm.shape == (6, 2, L)
    got, lengths = corpus.crops(cf, co, L, mix=(aug, draws), check=False, **kw)
    assert torch.equal(lengths, wlen) and torch.equal(bits(got), bits(want)) and not torch.equal(got[0], pcm[0])
    # and as one channel: the mono noise goes in as it is
    want1 = by_hand(pkg, corpus, noise, cf, co, draws, sample_rate=16000, mono=True)[0]
    got1 = corpus.crops(cf, co, L, mix=(aug, draws), check=False, sample_rate=16000, mono=True)[0]
    assert got1.shape == (6, 1, L) and torch.equal(bits(got1), bits(want1))


def test_features_and_normalize_follow_the_mixed_waveform(corpora):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.features import feature_lengths

    corpus, noise = corpora["sig"], corpora["mono"]
    spec = pkg.LogMel(RATE, 400, 160, 80, log="log10")
    cf, co = device_crops(torch, corpus, corpus.num_frames)
    aug = pkg.AddNoise(noise, (0, 15))
    draws = aug.draw(len(cf), L, generator=torch.Generator(device="cuda").manual_seed(3))
    wave, lengths = corpus.crops(cf, co, L, mix=(aug, draws), check=False)
    wave = wave.clone()
    feats, flen = corpus.crops(cf, co, L, mix=(aug, draws), features=spec, check=False)
    feats = feats.clone()
    assert torch.equal(bits(feats), bits(pkg.log_mel(wave, spec))) and torch.equal(flen, feature_lengths(lengths, 160))
    assert not torch.equal(feats, corpus.crops(cf, co, L, features=spec, check=False)[0])
    for how in (pkg.TopDb.whisper(), pkg.MeanVar()):
        got, glen = corpus.crops(cf, co, L, mix=(aug, draws), features=spec, normalize=how, check=False)
        assert torch.equal(glen, flen) and torch.equal(bits(got), bits(pkg.normalize(feats, how, flen))), how
    got, glen = corpus.crops(cf, co, L, mix=(aug, draws), normalize=pkg.MeanVar(), check=False)
    assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(pkg.normalize(wave, pkg.MeanVar(), lengths)))


def test_random_crops_are_reproducible_and_p_0_is_no_noise(corpora):
    import torch

    import alac.net_amd as pkg

    corpus, noise = corpora["sig"], corpora["stereo"]
    aug = pkg.AddNoise(noise, (5, 20), p=0.9)
    for dev in ("cuda", "cpu"):
        a = corpus.random_crops(8, L, generator=torch.Generator(device=dev).manual_seed(5), mix=aug)
        b = corpus.random_crops(8, L, generator=torch.Generator(device=dev).manual_seed(5), mix=aug)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), dev
        # the call's own two draws, then AddNoise.draw's four, from one generator
        g = torch.Generator(device=dev).manual_seed(5)
        plain = corpus.random_crops(8, L, generator=g)
        draws = aug.draw(8, L, sample_rate=RATE, generator=g)
        assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and torch.equal(plain[1], a[1])
        again = corpus.crops(a[2], a[3], L, mix=(aug, draws))
        assert torch.equal(bits(again[0]), bits(a[0])) and not torch.equal(a[0], plain[0]), dev
    none = pkg.AddNoise(noise, 10.0, p=0.0)
    g = torch.Generator(device="cuda").manual_seed(6)
    a = corpus.random_crops(8, L, generator=g, mix=none)
    assert torch.isnan(none.draw(8, L, generator=g)[2]).all()
    assert torch.equal(bits(a[0]), bits(corpus.crops(a[2], a[3], L)[0]))
    feats = corpus.random_crops(4, L, generator=torch.Generator().manual_seed(7), mix=aug, features=pkg.LogMel(RATE, 400, 160, 80))
    assert feats[0].shape == (4, 2, 80, 1 + L // 160)


def test_the_corpus_is_its_own_noise(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    cf, co = device_crops(torch, corpus, corpus.num_frames)
    with pkg.Corpus(corpora["sig_files"]) as twin:
        for kw in ({}, dict(sample_rate=16000, mono=True), dict(features=pkg.LogMel(RATE, 400, 160, 80))):
            if "sample_rate" in kw:
                cf, co = device_crops(torch, corpus, corpus.resampled_frames(16000))
            own, other = pkg.AddNoise(corpus, 3.0), pkg.AddNoise(twin, 3.0)
            draws = own.draw(len(cf), L, sample_rate=kw.get("sample_rate"), generator=torch.Generator(device="cuda").manual_seed(8))
            a, alen = corpus.crops(cf, co, L, mix=(own, draws), check=False, **kw)
            a = a.clone()
            st = corpus.last_status()[0].clone()
            b, blen = corpus.crops(cf, co, L, mix=(other, draws), check=False, **kw)
            assert torch.equal(bits(a), bits(b)) and torch.equal(alen, blen) and torch.equal(corpus.last_status()[0], st), kw
            assert not torch.equal(a, corpus.crops(cf, co, L, check=False, **kw)[0]), kw


def test_the_achieved_ratio_is_the_requested_one(corpora):
    """10 log10(Ps / P(y - x)) over the crop's v frames against the requested snr_db, on rows whose noise is not repeated
    (vn >= v).  The gain sets the noise's power over ITS vn frames, so where vn > v the expectation carries
    10 log10(Pn over vn / Pn over v), which is 0 where vn == v.  The tolerance is computed, not chosen: y - x is within dY of
    g n element by element (mix_host(bound=True), whose dY is dg's), so rms(y - x) is within rms(dY) of rms(g n), which is
    20 log10(1 +- rms(dY) / rms(g n)) decibels; and the ratio the kernel is given is 10^(-snr_db / 20) from a float32 power,
    good to 16 u = 2^-20 relative (two roundings of the exponent, scaled by |snr_db / 20| ln 10 <= 2.4, and the power's own
    two ulp of 2 u each, rounded up to a power of two), another 20 log10(1 + 2^-20)."""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.mix import mix_host, snr_ratio

    corpus, noise = corpora["sig"], corpora["mono"]
    B = 12
    g = torch.Generator(device="cuda").manual_seed(9)
    aug = pkg.AddNoise(noise, (0, 20))
    files = torch.randint(0, corpus.num_files, (B,), generator=g, device="cuda")
    offs = torch.zeros(B, dtype=torch.int64, device="cuda")
    offs[:3] = torch.tensor([int(corpus.num_frames[int(f)]) - 1000 for f in files[:3].tolist()], device="cuda")      # v = 1000
    # the noise files and offsets by hand: crops of 3000 frames of the first file, and the second file's 700 (repeated)
    draws = (torch.tensor([0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0], device="cuda"),
             torch.tensor([0, 500, 0, 100, 3000, 0, 3096, 7, 1500, 0, 2048, 1], device="cuda"), aug.draw(B, L, generator=g)[2])
    want, lengths, pcm, ncrops, nlen = by_hand(pkg, corpus, noise, files, offs, draws)
    got = corpus.crops(files, offs, L, mix=(aug, draws))[0]
    assert torch.equal(bits(got), bits(want))
    x, n, y = pcm.cpu().numpy(), ncrops.cpu().numpy(), got.cpu().numpy().astype(np.float64)
    snr = draws[2].cpu().numpy().astype(np.float64)
    a = snr_ratio(draws[2], B, pcm.device).cpu().numpy()
    spec, dY = mix_host(x, n, a, lengths.tolist(), nlen.tolist(), bound=True)
    rows = [b for b in range(B) if int(nlen[b]) >= int(lengths[b]) > 0]
    assert len(rows) >= 4 and any(int(nlen[b]) == int(lengths[b]) for b in rows) and any(int(nlen[b]) > int(lengths[b]) for b in rows)
    for b in rows:
        v, vn = int(lengths[b]), int(nlen[b])
        xs, d = x[b, :, :v].astype(np.float64), y[b, :, :v] - x[b, :, :v].astype(np.float64)
        achieved = 10 * np.log10((xs ** 2).mean() / (d ** 2).mean())
        n64 = n[b].astype(np.float64)
        expected = snr[b] + 10 * np.log10((n64[:, :vn] ** 2).mean() / (n64[:, :v] ** 2).mean())
        rel = np.sqrt((dY[b, :, :v] ** 2).mean()) / np.sqrt(((spec[b, :, :v] - xs) ** 2).mean())
        tol = -20 * np.log10(1 - rel) + 20 * np.log10(1 + 2.0 ** -20)
        print(f"crop {b}: v {v} vn {vn} requested {snr[b]:.4f} dB, expected {expected:.6f}, achieved {achieved:.6f}, tolerance {tol:.2e} dB")
        assert abs(achieved - expected) <= tol, (b, achieved, expected, tol)


def test_check_false_reads_nothing_back(corpora):
    # torch's sync debug mode raises on every synchronising call torch itself makes: in "error" mode the whole step runs through
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    spec = pkg.LogMel(16000, 400, 160, 80)
    for noise, kw in ((corpora["stereo"], {}), (corpora["rated"], dict(sample_rate=16000, mono=True, features=spec)), (corpus, {})):
        aug = pkg.AddNoise(noise, (5, 20), p=0.8)
        totals = corpus.num_frames if not kw else corpus.resampled_frames(16000)
        cf, co = device_crops(torch, corpus, totals)
        g = torch.Generator(device="cuda").manual_seed(10)
        draws = aug.draw(len(cf), L, sample_rate=kw.get("sample_rate"), generator=g)
        want, want_len = corpus.crops(cf, co, L, mix=(aug, draws), check=False, **kw)       # (also the first call's allocations)
        want = want.clone()
        corpus.random_crops(4, L, generator=g, mix=aug, check=False, **kw)
        out = torch.empty_like(want)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                want_len.cpu()
            got, lengths = corpus.crops(cf, co, L, mix=(aug, draws), check=False, **kw)
            got2, _ = corpus.crops(cf, co, L, mix=(aug, draws), check=False, out=out, **kw)
            drawn, _ = corpus.crops(cf, co, L, mix=aug, check=False, **kw)
            r = corpus.random_crops(4, L, generator=g, mix=aug, check=False, **kw)
            with pytest.raises(RuntimeError):
                corpus.crops(cf, co, L, mix=(aug, draws), check=True, **kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(bits(got), bits(want)) and got2 is out and torch.equal(bits(out), bits(want)) and torch.equal(lengths, want_len)
        assert drawn.shape == want.shape and r[0].shape[0] == 4


def test_what_cannot_be_mixed_is_refused_before_any_device_work(corpora):
    import torch

    import alac.net_amd as pkg

    corpus, noise = corpora["sig"], corpora["stereo"]
    aug = pkg.AddNoise(noise, 10.0)
    corpus.crops([0], [0], L)
    before = corpus.last_status()[0].clone()
    draws = aug.draw(1, L)
    with pkg.Corpus(corpora["sig_files"][:1]) as gone:
        closed = pkg.AddNoise(gone, 10.0)
    bad = [dict(mix=aug, dtype=torch.int32), dict(mix="noise"), dict(mix=noise), dict(mix=(aug,)), dict(mix=(aug, draws[:2])),
           dict(mix=(aug, (draws[0], draws[1], draws[0]))), dict(mix=(aug, tuple(t.cpu() for t in draws))), dict(mix=(aug, [1, 2, 3])),
           dict(mix=(draws, aug)), dict(mix=closed), dict(mix=(closed, draws))]
    for kw in bad:
        with pytest.raises(ValueError):
            corpus.crops([0], [0], L, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(1, L, **kw)
    with pytest.raises(ValueError):
        corpus.crops([0, 1], [0, 0], L, mix=(aug, draws))                       # one draw for two crops
    # a corpus whose rates differ has no rate of its own for the crops, and so none for the noise
    rated = corpora["rated"]
    with pytest.raises(ValueError):
        rated.crops([0], [0], L, mix=pkg.AddNoise(rated, 10.0))
    with pytest.raises(ValueError):
        rated.random_crops(1, L, mix=pkg.AddNoise(noise, 10.0))
    if torch.cuda.device_count() > 1:
        with pkg.Corpus(corpora["sig_files"][:1], device=1) as far:
            with pytest.raises(ValueError):
                corpus.crops([0], [0], L, mix=pkg.AddNoise(far, 10.0))
    assert torch.equal(corpus.last_status()[0], before)                          # nothing ran
    assert rated.crops([0], [0], L, sample_rate=16000, mix=pkg.AddNoise(corpus, 10.0))[0].shape == (1, 1, L)
