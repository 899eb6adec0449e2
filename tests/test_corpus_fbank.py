"""Corpus.crops(features=KaldiFbank(...)) on the GPU: the features of a crop are `alac.fbank` of that crop bit for bit (the same
kernel on the same data), at the corpus's rate as one channel, from files of different rates, with speed=, mix= and reverb= in
front and MeanVar and SpecAugment behind; the feature lengths are `fbank_lengths` of the lengths; a LogMel in the same place
gives what it gave; every new refusal comes before any device work.  What the kernel computes is tests/test_fbank.py's
subject."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
SAME = [(16000, 20000, 16, 4096), (16000, 9001, 24, 1024), (16000, 12000, 16, 1024)]
MIXED = [(44100, 20000, 16, 4096), (48000, 18001, 24, 1024), (16000, 12000, 16, 1024)]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    d = tmp_path_factory.mktemp("corpus_fbank")
    out = {}
    for name, spec in (("same", SAME), ("mixed", MIXED)):
        out[name] = []
        for i, (rate, frames, bits, fl) in enumerate(spec):
            path = str(d / f"{name}{i}_{rate}.m4a")
            pkg.save(path, signal(torch, rate, frames, 90 + i), rate, sample_size=bits, frame_length=fl)
            out[name].append(path)
    return out


def the_crops(totals):
    """Per file: its first frames, a middle, a crop that runs off the end, and the crop at the very end (length 0)"""
    crops = []
    for f, T in enumerate(totals):
        crops += [(f, 0), (f, int(T) // 3), (f, max(int(T) - L // 2, 0)), (f, int(T))]
    return [c[0] for c in crops], [c[1] for c in crops]


@pytest.mark.parametrize("snip", [True, False])
def test_features_of_crops_are_fbank_of_the_crops(paths, snip):
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiFbank(16000, snip_edges=snip)
    Tf = spec.frames(L)
    for tag, src, ckw, kw in (("16 kHz mono", paths["same"], {}, dict(sample_rate=16000, mono=True)),
                              ("mixed rates", paths["mixed"], dict(mixed_rates=True), dict(sample_rate=16000)),
                              ("mixed rates mono", paths["mixed"], dict(mixed_rates=True), dict(sample_rate=16000, mono=True))):
        with pkg.Corpus(src, **ckw) as corpus:
            totals = corpus.resampled_frames(16000)
            cf, co = the_crops(totals)
            pcm, lengths = corpus.crops(cf, co, L, **kw)
            want, want_len = pkg.fbank(pcm, spec, lengths)
            feats, flen = corpus.crops(cf, co, L, features=spec, **kw)
            Co = 1 if kw.get("mono") else corpus.channels
            assert feats.shape == (len(cf), Co, 80, Tf) and feats.dtype == torch.float32 and feats.is_cuda, tag
            assert torch.equal(feats.view(torch.int32), want.view(torch.int32)), tag
            assert torch.isfinite(feats).all(), tag
            lens = lengths.tolist()
            assert flen.dtype == torch.int64 and flen.is_cuda and torch.equal(flen, want_len), tag
            assert flen.tolist() == [spec.frames(n) for n in lens] == pkg.fbank_lengths(np.array(lens), spec).tolist(), tag
            # the crop at the file's end is silence: ln(2^-23) everywhere
            assert lens[3] == 0 and flen[3] == 0 and (feats[3] == feats[3].flatten()[0]).all()
            assert abs(float(feats[3].flatten()[0]) - np.log(2.0 ** -23)) < 1e-5
            # indices on the device, one of them outside the corpus: -1 and a row of silence
            d_f = torch.tensor(cf[:4] + [len(src)], device="cuda")
            d_o = torch.tensor(co[:4] + [0], device="cuda")
            f2, l2 = corpus.crops(d_f, d_o, L, features=spec, check=False, **kw)
            assert l2.tolist() == flen.tolist()[:4] + [-1] and torch.equal(f2[:4], feats[:4]), tag
            r = corpus.random_crops(5, L, check=False, features=spec, **kw)
            assert r[0].shape == (5, Co, 80, Tf) and r[1].shape == (5,) and r[2].shape == (5,) and r[3].shape == (5,), tag
            out = torch.full_like(feats, float("nan"))
            got = corpus.crops(cf, co, L, features=spec, out=out, **kw)[0]
            assert got is out and torch.equal(out, feats), tag


def test_stages_in_front_and_behind(paths):
    """speed=, mix= and reverb= in front with given draws, MeanVar and SpecAugment behind: the call with features= is the call
    without it, then fbank, normalize and spec_augment"""
    import torch

    import alac.net_amd as pkg

    spec = pkg.KaldiFbank(16000)
    kw = dict(sample_rate=16000, mono=True, check=False)
    with pkg.Corpus(paths["mixed"], mixed_rates=True) as corpus, pkg.Corpus(paths["same"]) as other:
        B = 6
        g = torch.Generator(device="cuda").manual_seed(3)
        _, _, files, offs = corpus.random_crops(B, L, generator=g, **kw)
        speed, add, rev = pkg.SpeedPerturb((0.9, 1.0, 1.1)), pkg.AddNoise(other, (5, 20)), pkg.Reverb(other, max_seconds=0.05)
        front = dict(speed=(speed, speed.draw(B, generator=g)), mix=(add, add.draw(B, L, sample_rate=16000, generator=g)),
                     reverb=(rev, rev.draw(B, generator=g)))
        for names in ((), ("speed",), ("mix",), ("reverb",), ("speed", "mix", "reverb")):
            on = {k: front[k] for k in names}
            pcm, lengths = corpus.crops(files, offs, L, **on, **kw)
            want, want_len = pkg.fbank(pcm.clone(), spec, lengths)
            feats, flen = corpus.crops(files, offs, L, features=spec, **on, **kw)
            assert torch.equal(feats.view(torch.int32), want.view(torch.int32)) and torch.equal(flen, want_len), names
            how, aug = pkg.MeanVar(), pkg.SpecAugment(freq_masks=2, freq_width=10, time_masks=2, time_width=5, time_warp=3)
            normed = pkg.normalize(want.clone(), how, want_len)
            got = corpus.crops(files, offs, L, features=spec, normalize=how, **on, **kw)
            assert torch.equal(got[0].view(torch.int32), normed.view(torch.int32)) and torch.equal(got[1], want_len), names
            draws = aug.draw(spec.n_mels, want_len, generator=g)
            masked = pkg.spec_augment(normed.clone(), (aug, draws), want_len)
            got = corpus.crops(files, offs, L, features=spec, normalize=how, augment=(aug, draws), **on, **kw)
            assert torch.equal(got[0].view(torch.int32), masked.view(torch.int32)), names
            assert not torch.equal(masked, normed)
        # random_crops draws the SpecAugment for the fbank lengths: reproducible from a seed
        runs = [corpus.random_crops(B, L, generator=torch.Generator(device="cuda").manual_seed(11), features=spec, normalize=how,
                                    augment=aug, **kw) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*runs)) and runs[0][0].shape == (B, 1, 80, spec.frames(L))


def test_a_logmel_gives_what_it_gave(paths):
    import torch

    import alac.net_amd as pkg

    spec = pkg.LogMel(16000, 400, 160, 80)
    with pkg.Corpus(paths["same"]) as corpus:
        cf, co = the_crops(corpus.num_frames)
        pcm, lengths = corpus.crops(cf, co, L, mono=True)
        want, want_len = pkg.log_mel(pcm, spec, lengths)
        feats, flen = corpus.crops(cf, co, L, mono=True, features=spec)
        assert torch.equal(feats.view(torch.int32), want.view(torch.int32)) and torch.equal(flen, want_len)
        assert flen.tolist() == [n // 160 + 1 for n in lengths.tolist()]
        with pytest.raises(ValueError, match="more than n_fft // 2 = 200"):
            corpus.crops([0], [0], 200, features=spec)


def test_new_refusals_come_before_any_device_work(paths):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(paths["same"]) as corpus, pkg.Corpus(paths["mixed"], mixed_rates=True) as mixed:
        corpus.crops([0], [0], 500)
        last = corpus._last
        k16, k8 = pkg.KaldiFbank(16000), pkg.KaldiFbank(8000)
        centred = pkg.KaldiFbank(16000, snip_edges=False)
        warp = pkg.SpecAugment(time_warp=5)
        for kw in (dict(features=k8), dict(features=k16, sample_rate=8000), dict(features=k16, dtype=torch.int32),
                   dict(features=k16, dtype="int32"), dict(features=k16, num_frames=399), dict(features=k16, num_frames=0),
                   dict(features=centred, num_frames=79), dict(features=k16, augment=warp, num_frames=400 + 160 * 16384),
                   dict(features="fbank")):
            n = kw.pop("num_frames", 1000)
            with pytest.raises(ValueError):
                corpus.crops([0], [0], n, **kw)
            with pytest.raises(ValueError):
                corpus.random_crops(2, n, **kw)
        with pytest.raises(ValueError, match="no feature frame"):
            corpus.crops([0], [0], 399, features=k16)
        with pytest.raises(ValueError, match="a time warp takes at most 16384"):
            corpus.crops([0], [0], 400 + 160 * 16384, features=k16, augment=warp)
        with pytest.raises(ValueError, match="LogMel or a fbank.KaldiFbank"):
            corpus.crops([0], [0], 1000, None, None, True, 16000)     # a rate where the features go
        assert corpus._last == last and corpus._ft_scratch is None
        with pytest.raises(ValueError, match="sample_rate="):
            mixed.crops([0], [0], 1000, features=k16)
        # the shortest crops
        assert corpus.crops([0], [0], 400, features=k16)[0].shape == (1, 2, 80, 1)
        assert corpus.crops([0], [0], 80, features=centred)[0].shape == (1, 2, 80, 1)
        empty, n0 = corpus.crops([], [], 1000, features=k16)
        assert empty.shape == (0, 2, 80, 4) and n0.shape == (0,)
