"""Corpus.crops(features=KaldiMfcc, deltas=, vad=, normalize=SlidingMeanVar.xvector(), augment=) on the GPU, on a small synthetic
corpus built as tests/test_corpus_mfcc.py builds its own, of alternating loud and silent stretches, so that the VAD has something
to cut: the result is bit for bit the free functions -- vad_energy, normalize, select_frames, spec_augment -- applied in that
order to what the same call returns without vad= and normalize=; the lengths are the voiced counts; a crop outside the corpus
keeps -1; the new refusals come before any device work.  What the kernels compute is tests/test_sliding.py's and
tests/test_vad.py's subject."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 16000
RATE = 16000
FILES = [(40000, 16, 4096, 1), (23001, 24, 1024, 2), (30000, 16, 1024, 3)]


def stretches(torch, frames, seed):
    """Stereo float32 [2, frames]: stretches of 2400 frames, tones at 0.3 and noise at 1e-4 in turn"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / RATE
    loud = (np.arange(frames) // 2400) % 2 == seed % 2
    x = np.stack([np.where(loud, 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + c), 0.0)
                  + 1e-4 * rng.standard_normal(frames) for c in (0, 1)])
    return torch.from_numpy(x.astype(np.float32)).to("cuda")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    d = tmp_path_factory.mktemp("corpus_vad")
    paths = []
    for i, (frames, bits, fl, seed) in enumerate(FILES):
        paths.append(str(d / f"vad{i}.m4a"))
        pkg.save(paths[-1], stretches(torch, frames, seed), RATE, sample_size=bits, frame_length=fl)
    with pkg.Corpus(paths) as c:
        yield c


def device_crops(torch, corpus):
    """Per file its first frames, a middle and a crop that runs off the end; the last crop is outside the corpus"""
    cf, co = [], []
    for f, T in enumerate(corpus.num_frames):
        cf += [f, f, f]
        co += [0, int(T) // 3, int(T) - L // 2]
    return torch.tensor(cf + [corpus.num_files], device="cuda"), torch.tensor(co + [0], device="cuda")


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


VAD = dict(energy_threshold=0.0, energy_mean_scale=1.0, frames_context=2, proportion_threshold=0.12)     # the bar is the mean energy


def test_crops_are_the_free_functions_in_kaldis_order(corpus):
    import torch

    import alac.net_amd as pkg

    spec, deltas, how = pkg.KaldiMfcc(RATE, n_mels=30, n_ceps=30), pkg.Deltas(1, 2), pkg.SlidingMeanVar.xvector()
    policy = pkg.SpecAugment(freq_masks=1, freq_width=5, time_masks=1, time_width=10)
    d_f, d_o = device_crops(torch, corpus)
    for mono, line in ((True, 0), (False, 3)):
        vad = pkg.EnergyVad(line=line, **VAD) if line == 0 else pkg.EnergyVad(-100.0, 0.0, 1, 1.0, line=line)
        kw = dict(mono=mono, features=spec, deltas=deltas, check=False)
        base, blen = corpus.crops(d_f, d_o, L, **kw)
        base = base.clone()
        draws = policy.draw(base.shape[2], blen)
        # the composition: the decision on the raw features, the CMVN over all frames, the selection, then SpecAugment
        mask = pkg.vad_energy(base, vad, blen)
        normed = pkg.normalize(base, how, blen)
        sel, new = pkg.select_frames(normed, mask, blen)
        want = pkg.spec_augment(sel, (policy, draws), new)
        got, glen = corpus.crops(d_f, d_o, L, vad=vad, normalize=how, augment=(policy, draws), **kw)
        assert same_bits(torch, got, want) and torch.equal(glen, new), (mono, line)
        # each alone, and into `out`
        got_v, len_v = corpus.crops(d_f, d_o, L, vad=vad, **kw)
        sel_v, new_v = pkg.select_frames(base, mask, blen)
        assert same_bits(torch, got_v, sel_v) and torch.equal(len_v, new_v) and torch.equal(len_v, new)
        got_n, len_n = corpus.crops(d_f, d_o, L, normalize=how, **kw)
        assert same_bits(torch, got_n, normed) and torch.equal(len_n, blen)
        out = torch.full_like(base, float("nan"))
        res = corpus.crops(d_f, d_o, L, vad=vad, normalize=how, out=out, **kw)
        assert res[0] is out and same_bits(torch, out, sel) and torch.equal(res[1], new)
        # the lengths are the voiced counts; a crop outside the corpus keeps -1 and is zeros
        before, after = blen.tolist(), glen.tolist()
        assert before[-1] == -1 and after[-1] == -1 and (got[-1] == 0).all()
        if line == 0:
            for b, (v0, v1) in enumerate(zip(before[:-1], after[:-1])):
                assert 0 < v1 < v0, (b, v0, v1)
                assert (got[b, ..., v1:] == 0).all() and torch.isfinite(got[b]).all()
            assert after[:-1] == mask.sum(dim=1).tolist()[:-1]
        else:                                                       # a bar of -100 on every frame: all voiced, a copy
            assert after == before and same_bits(torch, sel, normed)
        # one call on a side stream gives the same bits
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            side, side_len = corpus.crops(d_f, d_o, L, vad=vad, normalize=how, augment=(policy, draws), **kw)
        s.synchronize()
        assert same_bits(torch, side, got) and torch.equal(side_len, glen)
    # PCM takes a SlidingMeanVar too
    pcm, plen = corpus.crops(d_f, d_o, 3000, check=False)
    pcm = pcm.clone()
    got = corpus.crops(d_f, d_o, 3000, check=False, normalize=pkg.SlidingMeanVar(64, 10))[0]
    assert same_bits(torch, got, pkg.normalize(pcm, pkg.SlidingMeanVar(64, 10), plen))


def test_random_crops_reproduce_and_read_nothing_back(corpus):
    import torch

    import alac.net_amd as pkg

    spec, how, vad = pkg.KaldiMfcc(RATE, n_mels=30, n_ceps=30), pkg.SlidingMeanVar.xvector(), pkg.EnergyVad(**VAD)
    policy = pkg.SpecAugment(freq_masks=1, freq_width=5, time_masks=1, time_width=10)
    kw = dict(sample_rate=RATE, mono=True, features=spec, vad=vad, normalize=how, check=False)
    a = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(11), augment=policy, **kw)
    b = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(11), augment=policy, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].shape == (6, 1, 30, spec.frames(L)) and a[1].dtype == torch.int64 and a[1].is_cuda
    plain = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(11), **kw)
    assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and torch.equal(plain[1], a[1])
    want = corpus.crops(plain[2], plain[3], L, **kw)
    assert same_bits(torch, plain[0], want[0]) and torch.equal(plain[1], want[1])
    full = corpus.crops(plain[2], plain[3], L, sample_rate=RATE, mono=True, features=spec, check=False)[1]
    assert ((plain[1] > 0) & (plain[1] < full)).all()
    # the README's step
    res = corpus.random_crops(8, 48000, sample_rate=16000, mono=True, features=spec, vad=pkg.EnergyVad.voxceleb(), normalize=how, check=False)
    assert res[0].shape == (8, 1, 30, 298) and (res[1] <= 298).all()


def test_corpus_refuses_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiMfcc(RATE)
    for kw in (dict(vad=pkg.EnergyVad()),                                               # no features=
               dict(vad="energy", features=spec), dict(vad=pkg.EnergyVad(line=13), features=spec),
               dict(vad=pkg.EnergyVad(line=26), features=spec, deltas=pkg.Deltas(1, 2)),
               dict(normalize=pkg.SlidingMeanVar(), dtype=torch.int32),
               dict(normalize=pkg.SlidingMeanVar(8000, 100))):                          # 16385 frames of PCM through the ring
        with pytest.raises(ValueError):
            corpus.crops([0], [0], 16385 if "features" not in kw and "vad" not in kw else L, **kw)
    with pytest.raises(ValueError):
        corpus.random_crops(2, L, vad=pkg.EnergyVad())
    assert corpus.crops([0], [0], L, features=spec, deltas=pkg.Deltas(1, 2), vad=pkg.EnergyVad(line=25))[0].shape[2] == 26
