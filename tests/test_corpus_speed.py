"""Corpus.crops(..., speed=) on the GPU: the four files of tests/test_corpus_mixed_rates.py played at 0.9 / 1.0 / 1.1, every
crop against its file, as `load` returns it, resampled as a whole by the float64 specification with speed.ratio(file rate,
factor, 16000) and cut -- within speed.speed_bound; at factor 1 the specification and bound of the call without speed= --; the crops at factor 1 bit for bit the crops without speed=; the draws of
random_crops; the host tier; features behind it; and crops outside the corpus."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGET = 16000
L = 1500
# (sample rate, frames, bits, frame length)
SPEC = [(44100, 20000, 16, 4096), (48000, 18001, 24, 1024), (16000, 12000, 16, 1024), (22050, 15000, 16, 4096)]


def signal(torch, rate, frames, seed):
    """A stereo signal that compresses: a few tones and a little noise, float32 [2, frames] on the device"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / rate
    x = np.stack([0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + c) + 0.01 * rng.standard_normal(frames) for c in (0, 1)])
    return torch.from_numpy(x.astype(np.float32)).to("cuda")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The four files (written by `save`), the policy, and refs[mono][f][k]: (file f at factor k resampled by the
    specification, its bound)"""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_host
    from alac.net_amd.speed import SpeedPerturb, ratio, speed_bound, speed_host

    d = tmp_path_factory.mktemp("speed")
    sp = SpeedPerturb()
    paths, refs = [], {False: [], True: []}
    for i, (rate, frames, bits, fl) in enumerate(SPEC):
        path = str(d / f"f{i}_{rate}.m4a")
        pkg.save(path, signal(torch, rate, frames, 50 + i), rate, sample_size=bits, frame_length=fl)
        paths.append(path)
        x = pkg.load(path)[0].cpu().numpy().astype(np.float64)
        N = 3 if rate == TARGET else 2 * ratio(rate, 1, TARGET)[2] + 1
        for mono in (False, True):
            # factor 1 is the crop without speed=: the table kernels' specification and bound (tests/test_corpus_mixed_rates.py)
            plain = (resample_host(x, rate, TARGET, mono=mono), (N + 2) * 2.0 ** -24 * resample_host(x, rate, TARGET, mono=mono, magnitude=True))
            refs[mono].append([plain if f == 1 else (speed_host(x, *ratio(rate, f, TARGET), mono=mono),
                                                     speed_bound(x, *ratio(rate, f, TARGET), mono=mono)) for f in sp.factors])
    return paths, sp, refs


def the_crops(Ty):
    """Per file (a row of Ty) and factor: the first frames, the last 700 running past the end, and a middle"""
    cf, co, ck = [], [], []
    for f, row in enumerate(Ty):
        for k, n in enumerate(row):
            for o in (0, int(n) - 700, int(n) // 2 + 3):
                cf.append(f), co.append(o), ck.append(k)
    return cf, co, ck


def check_crops(pcm, lengths, refs, cf, co, ck, tag):
    got, lens = pcm.cpu().numpy().astype(np.float64), lengths.tolist()
    worst = 0.0
    for b, (f, o, k) in enumerate(zip(cf, co, ck)):
        want, tol = refs[f][k]
        n = min(L, want.shape[1] - o)
        assert lens[b] == n, (tag, b, lens[b], n)
        err = np.abs(got[b, :, :n] - want[:, o:o + n])
        worst = max(worst, float(np.max(err / np.maximum(tol[:, o:o + n], 1e-300))))
        assert (err <= tol[:, o:o + n]).all(), (tag, b, f, o, k, float(err.max()))
        assert not got[b, :, n:].any() and got[b, :, :n].any(), (tag, b)
    print(f"{tag}: {len(cf)} crops, worst err / bound {worst:.3f}")


def dev(torch, v):
    return torch.tensor(v, device="cuda", dtype=torch.int64)


def test_single_rate_corpus_with_given_draws(files):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.speed import ratio

    paths, sp, refs = files
    with pkg.Corpus(paths[:1]) as corpus:
        Ty = corpus.resampled_frames(TARGET, speed=sp)
        assert Ty.shape == (1, 3) and Ty.dtype == np.int64
        assert Ty[0].tolist() == [-(-b * 20000 // a) for a, b, _ in (ratio(44100, f, TARGET) for f in sp.factors)]
        assert Ty[0, 1] == corpus.resampled_frames(TARGET)[0]
        cf, co, ck = the_crops(Ty)
        for mono in (False, True):
            pcm, lengths = corpus.crops(cf, co, L, sample_rate=TARGET, mono=mono, speed=(sp, dev(torch, ck)))
            assert pcm.shape == (9, 1 if mono else 2, L) and pcm.dtype == torch.float32 and lengths.dtype == torch.int64
            check_crops(pcm, lengths, [r for r in refs[mono][:1]], cf, co, ck, f"44.1 kHz alone, mono={mono}")
            assert lengths.tolist()[1] == 700
        # refusals, before any device work
        for kw in (dict(speed=0.9), dict(speed=(sp, ck)), dict(speed=(sp, dev(torch, ck).float())), dict(speed=(sp, dev(torch, ck).cpu())),
                   dict(speed=sp, dtype=torch.int32), dict(speed=(sp, dev(torch, ck[:3])))):
            with pytest.raises(ValueError):
                corpus.crops(cf, co, L, sample_rate=TARGET, **kw)
        with pytest.raises(ValueError):       # a host offset past the file's largest Ty over the factors
            corpus.crops([0], [int(Ty.max()) + 1], L, sample_rate=TARGET, speed=(sp, dev(torch, [0])))


def test_mixed_rate_corpus_with_given_draws(files):
    import torch

    import alac.net_amd as pkg

    paths, sp, refs = files
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        Ty = corpus.resampled_frames(TARGET, speed=sp)
        assert Ty.shape == (4, 3) and [[r[k][0].shape[1] for k in range(3)] for r in refs[True]] == Ty.tolist()
        cf, co, ck = the_crops(Ty)
        pcm, lengths = corpus.crops(cf, co, L, sample_rate=TARGET, mono=True, speed=(sp, dev(torch, ck)))
        assert pcm.shape == (36, 1, L)
        check_crops(pcm, lengths, refs[True], cf, co, ck, "four rates, mono")
        # device indices and out= holding garbage: the same crops
        out = torch.full_like(pcm, 12345.0)
        pcm2, lengths2 = corpus.crops(dev(torch, cf), dev(torch, co), L, sample_rate=TARGET, mono=True, speed=(sp, dev(torch, ck)), out=out)
        assert pcm2 is out and torch.equal(pcm2, pcm) and torch.equal(lengths2, lengths)


def test_factor_one_is_the_call_without_speed(files):
    import torch

    import alac.net_amd as pkg

    paths, sp, _ = files
    cases = [(paths[:1], {}, dict(sample_rate=TARGET)), (paths[:1], {}, dict(sample_rate=TARGET, mono=True)),
             (paths, dict(mixed_rates=True), dict(sample_rate=TARGET, mono=True)), (paths, dict(mixed_rates=True), dict(sample_rate=TARGET)),
             (paths[2:3], {}, {}), (paths[:1], {}, dict(mono=True))]
    for srcs, how, kw in cases:
        with pkg.Corpus(srcs, **how) as corpus:
            Ty = corpus.resampled_frames(kw.get("sample_rate"), speed=sp)
            cf, co, ck = the_crops(Ty)
            pcm, lengths = corpus.crops(cf, co, L, speed=(sp, dev(torch, ck)), **kw)
            rows = [b for b in range(len(ck)) if ck[b] == sp.one]
            assert len(rows) == 3 * len(srcs)
            plain, plain_len = corpus.crops([cf[b] for b in rows], [co[b] for b in rows], L, **kw)
            assert torch.equal(pcm[rows], plain) and torch.equal(lengths[rows], plain_len), kw
            others = [b for b in range(len(ck)) if ck[b] != sp.one]
            assert pcm[others].abs().sum() > 0
            # only factor 1 drawn: the whole call
            ones = dev(torch, [sp.one] * len(rows))
            again, again_len = corpus.crops([cf[b] for b in rows], [co[b] for b in rows], L, speed=(sp, ones), **kw)
            assert torch.equal(again, plain) and torch.equal(again_len, plain_len)


def test_random_crops_draws(files):
    import torch

    import alac.net_amd as pkg

    paths, sp, _ = files
    g = lambda: torch.Generator(device="cuda").manual_seed(11)
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        one = corpus.random_crops(24, L, sample_rate=TARGET, speed=sp, generator=g())
        two = corpus.random_crops(24, L, sample_rate=TARGET, speed=sp, generator=g())
        assert all(torch.equal(x, y) for x, y in zip(one, two))
        pcm, lengths, cf, co = one
        # the draws recomputed from the same seed: behind the call's own two
        gen = g()
        f2 = torch.randint(0, corpus.num_files, (24,), generator=gen, device="cuda", dtype=torch.int64)
        u = torch.rand(24, generator=gen, device="cuda", dtype=torch.float64)
        k = sp.draw(24, generator=gen, device="cuda")
        assert torch.equal(f2, cf) and len(set(k.tolist())) == 3
        Ty = torch.from_numpy(corpus.resampled_frames(TARGET, speed=sp)).to("cuda")
        span = (Ty[cf, k] - L).clamp(min=0)
        assert torch.equal(co, torch.minimum(torch.floor(u * (span + 1).double()).long(), span))
        same, same_len = corpus.crops(cf, co, L, sample_rate=TARGET, speed=(sp, k))
        assert torch.equal(same, pcm) and torch.equal(same_len, lengths) and (lengths == L).all()
        # without speed= the same seed gives today's files and offsets
        _, _, pf, po = corpus.random_crops(24, L, sample_rate=TARGET, generator=g())
        Tp = torch.from_numpy(corpus.resampled_frames(TARGET)).to("cuda")
        span = (Tp[cf] - L).clamp(min=0)
        assert torch.equal(pf, cf) and torch.equal(po, torch.minimum(torch.floor(u * (span + 1).double()).long(), span))


def test_host_tier_gives_the_same_bits(files):
    import torch

    import alac.net_amd as pkg

    paths, sp, _ = files
    with pkg.Corpus(paths, mixed_rates=True) as corpus, pkg.Corpus(paths, mixed_rates=True, hbm_bytes=0) as tiered:
        assert tiered.tier_bytes[0] == 0
        cf, co, ck = the_crops(corpus.resampled_frames(TARGET, speed=sp))
        a = corpus.crops(cf, co, L, sample_rate=TARGET, speed=(sp, dev(torch, ck)))
        b = tiered.crops(cf, co, L, sample_rate=TARGET, speed=(sp, dev(torch, ck)))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_features_behind_speed(files):
    import torch

    import alac.net_amd as pkg

    paths, sp, _ = files
    mel = pkg.LogMel(TARGET)
    with pkg.Corpus(paths[:1]) as corpus:
        cf, co, ck = the_crops(corpus.resampled_frames(TARGET, speed=sp))
        pcm, lengths = corpus.crops(cf, co, L, sample_rate=TARGET, speed=(sp, dev(torch, ck)))
        feats, flen = corpus.crops(cf, co, L, sample_rate=TARGET, speed=(sp, dev(torch, ck)), features=mel)
        want, wlen = pkg.log_mel(pcm, mel, lengths)
        assert torch.equal(feats, want) and torch.equal(flen, wlen)


def test_crops_outside_the_corpus(files):
    import torch

    import alac.net_amd as pkg

    paths, sp, _ = files
    with pkg.Corpus(paths[:1]) as corpus:
        Ty = corpus.resampled_frames(TARGET, speed=sp)
        cf, ck = dev(torch, [0, 0, 0, 0]), dev(torch, [0, 2, 2, 3])
        co = dev(torch, [5, int(Ty[0, 2]) + 1, int(Ty[0, 2]), 0])            # crop 1 is past Ty[0, 2] (inside Ty[0, 0]); crop 3 draws no factor
        with pytest.raises(ValueError, match="crop 1"):
            corpus.crops(cf, co, L, sample_rate=TARGET, speed=(sp, ck))
        pcm, lengths = corpus.crops(cf, co, L, sample_rate=TARGET, speed=(sp, ck), check=False)
        assert lengths.tolist() == [L, -1, 0, -1]
        assert pcm[0].any() and not pcm[1:].any()
