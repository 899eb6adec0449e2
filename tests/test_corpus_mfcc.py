"""Corpus.crops(features=KaldiMfcc(...), deltas=Deltas(...)) on the GPU, on a small synthetic corpus as
tests/test_corpus_fbank.py builds one: the features of a crop are `alac.mfcc` of that crop bit for bit, with deltas=
`add_deltas` of that with the feature lengths, with MeanVar and SpecAugment behind them the public calls composed in that
order; a crop outside the corpus keeps its features as computed and gets zero deltas; the new refusals come before any device
work.  What the kernels compute is tests/test_mfcc.py's and tests/test_deltas.py's subject."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
SAME = [(16000, 20000, 16, 4096), (16000, 9001, 24, 1024), (16000, 12000, 16, 1024)]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    d = tmp_path_factory.mktemp("corpus_mfcc")
    paths = []
    for i, (rate, frames, bits, fl) in enumerate(SAME):
        paths.append(str(d / f"same{i}_{rate}.m4a"))
        pkg.save(paths[-1], signal(torch, rate, frames, 70 + i), rate, sample_size=bits, frame_length=fl)
    with pkg.Corpus(paths) as c:
        yield c


def the_crops(totals):
    """Per file: its first frames, a middle, a crop that runs off the end, and the crop at the very end (length 0)"""
    crops = []
    for f, T in enumerate(totals):
        crops += [(f, 0), (f, int(T) // 3), (f, max(int(T) - L // 2, 0)), (f, int(T))]
    return [c[0] for c in crops], [c[1] for c in crops]


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kw", [dict(), dict(snip_edges=False, use_energy=True)], ids=["default", "centred-energy"])
def test_features_and_deltas_of_crops(corpus, kw):
    import torch

    import alac.net_amd as pkg

    spec, deltas = pkg.KaldiMfcc(16000, **kw), pkg.Deltas()
    Tf = spec.frames(L)
    cf, co = the_crops(corpus.num_frames)
    for mono in (True, False):
        Co = 1 if mono else corpus.channels
        pcm, lengths = corpus.crops(cf, co, L, mono=mono)
        want, want_len = pkg.mfcc(pcm, spec, lengths)
        feats, flen = corpus.crops(cf, co, L, mono=mono, features=spec)
        assert feats.shape == (len(cf), Co, 13, Tf) and feats.dtype == torch.float32 and feats.is_cuda
        assert same_bits(torch, feats, want) and torch.isfinite(feats).all()
        assert flen.dtype == torch.int64 and torch.equal(flen, want_len) and flen.tolist() == [spec.frames(n) for n in lengths.tolist()]
        stacked, slen = corpus.crops(cf, co, L, mono=mono, features=spec, deltas=deltas)
        assert stacked.shape == (len(cf), Co, 39, Tf) and torch.equal(slen, flen)
        assert same_bits(torch, stacked, pkg.add_deltas(feats, deltas, flen))
        assert same_bits(torch, stacked[:, :, :13], feats) and stacked[0, :, 13:].any()
        assert (stacked[3, :, 13:] == 0).all()                       # the crop at the file's end: no frame, zero deltas
        out = torch.full_like(stacked, float("nan"))
        got = corpus.crops(cf, co, L, mono=mono, features=spec, deltas=deltas, out=out)[0]
        assert got is out and torch.equal(out, stacked)
        # indices on the device, one of them outside the corpus: feat_lengths -1, the row static as computed, deltas zero
        d_f = torch.tensor(cf[:4] + [corpus.num_files], device="cuda")
        d_o = torch.tensor(co[:4] + [0], device="cuda")
        s2, l2 = corpus.crops(d_f, d_o, L, mono=mono, features=spec, deltas=deltas, check=False)
        f2 = corpus.crops(d_f, d_o, L, mono=mono, features=spec, check=False)[0]
        assert l2.tolist() == flen.tolist()[:4] + [-1] and same_bits(torch, s2[:4], stacked[:4])
        assert same_bits(torch, s2[4, :, :13], f2[4]) and (s2[4, :, 13:] == 0).all()
        # a KaldiFbank takes deltas as well
        fb = pkg.KaldiFbank(16000, n_mels=23)
        got = corpus.crops(cf, co, L, mono=mono, features=fb, deltas=pkg.Deltas(1, 3))
        want_fb = corpus.crops(cf, co, L, mono=mono, features=fb)
        assert got[0].shape == (len(cf), Co, 46, fb.frames(L)) and same_bits(torch, got[0], pkg.add_deltas(want_fb[0], pkg.Deltas(1, 3), want_fb[1]))


def test_normalize_and_augment_behind_the_deltas(corpus):
    import torch

    import alac.net_amd as pkg

    spec, deltas = pkg.KaldiMfcc(16000), pkg.Deltas()
    how, aug = pkg.MeanVar(), pkg.SpecAugment(freq_masks=2, freq_width=6, time_masks=2, time_width=4, time_warp=2)
    cf, co = the_crops(corpus.num_frames)
    kw = dict(mono=True, features=spec)
    feats, flen = corpus.crops(cf, co, L, **kw)
    stacked = pkg.add_deltas(feats, deltas, flen)
    normed = pkg.normalize(stacked.clone(), how, flen)
    got = corpus.crops(cf, co, L, deltas=deltas, normalize=how, **kw)
    assert same_bits(torch, got[0], normed) and torch.equal(got[1], flen) and not torch.equal(normed, stacked)
    g = torch.Generator(device="cuda").manual_seed(5)
    draws = aug.draw(39, flen, generator=g)
    masked = pkg.spec_augment(normed.clone(), (aug, draws), flen)
    got = corpus.crops(cf, co, L, deltas=deltas, normalize=how, augment=(aug, draws), **kw)
    assert same_bits(torch, got[0], masked) and not torch.equal(masked, normed)
    # without deltas the same two stages see 13 lines
    got = corpus.crops(cf, co, L, normalize=how, **kw)
    assert same_bits(torch, got[0], pkg.normalize(feats.clone(), how, flen))
    # random_crops accepts both keywords; its SpecAugment is drawn for 39 lines, reproducibly from a seed
    runs = [corpus.random_crops(6, L, generator=torch.Generator(device="cuda").manual_seed(11), deltas=deltas, normalize=how,
                                augment=aug, check=False, **kw) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and runs[0][0].shape == (6, 1, 39, spec.frames(L))
    r = corpus.random_crops(4, L, check=False, deltas=deltas, **kw)
    plain = corpus.crops(r[2], r[3], L, check=False, **kw)
    assert same_bits(torch, r[0], pkg.add_deltas(plain[0], deltas, plain[1])) and torch.equal(r[1], plain[1])


def test_new_refusals_come_before_any_device_work(corpus):
    import torch

    import alac.net_amd as pkg

    corpus.crops([0], [0], 500)
    last, scratch = corpus._last, corpus._delta_scratch
    corpus._delta_scratch = None
    m16, m8 = pkg.KaldiMfcc(16000), pkg.KaldiMfcc(8000)
    for kw in (dict(deltas=pkg.Deltas()), dict(deltas=pkg.Deltas(), normalize=pkg.MeanVar()), dict(features=m16, deltas=2),
               dict(features=m16, deltas="deltas"), dict(features=m8, deltas=pkg.Deltas()), dict(features=m16, dtype=torch.int32),
               dict(features=m16, num_frames=399), dict(features=m16, deltas=pkg.Deltas(), num_frames=399)):
        kw = dict(kw)
        n = kw.pop("num_frames", 1000)
        with pytest.raises(ValueError):
            corpus.crops([0], [0], n, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(2, n, **kw)
    with pytest.raises(ValueError, match="need features="):
        corpus.crops([0], [0], 1000, deltas=pkg.Deltas())
    with pytest.raises(ValueError, match="out must be"):
        corpus.crops([0], [0], 1000, features=m16, deltas=pkg.Deltas(), out=torch.empty(1, 2, 13, 4, device="cuda"))
    assert corpus._last == last and corpus._delta_scratch is None
    corpus._delta_scratch = scratch
    assert corpus.crops([0], [0], 400, features=m16, deltas=pkg.Deltas())[0].shape == (1, 2, 39, 1)
    empty, n0 = corpus.crops([], [], 1000, features=m16, deltas=pkg.Deltas())
    assert empty.shape == (0, 2, 39, 4) and n0.shape == (0,)
