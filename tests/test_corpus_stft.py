"""Corpus.crops(features=Spectrogram) on the GPU: the features of a crop are `spectrogram` of that crop bit for bit (the same
kernel on the same data), at the corpus's own rate with two channels, at another rate and as mono; the feature lengths; the
stages behind it -- deltas=, normalize=, a Pcen, augment= -- as behind a LogMel; f0=Yin.like(spec) on the feature frames; the
complex kind's refusals.  What the kernel computes is tests/test_stft.py's subject."""
import pytest

pytestmark = pytest.mark.gpu

L = 3000
SAME = [(44100, 20000, 16, 4096), (44100, 9001, 24, 1024)]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    d = tmp_path_factory.mktemp("corpus_stft")
    out = []
    for i, (rate, frames, bits, fl) in enumerate(SAME):
        path = str(d / f"same{i}_{rate}.m4a")
        pkg.save(path, signal(torch, rate, frames, 90 + i), rate, sample_size=bits, frame_length=fl)
        out.append(path)
    return out


def the_spec(pkg, rate, **kw):
    kw.setdefault("filterbank", pkg.mel_filterbank(rate, 512, 24))
    return pkg.Spectrogram(rate, 512, 160, **kw)


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def the_crops(totals):
    crops = []
    for f, T in enumerate(totals):
        crops += [(f, 0), (f, int(T) // 3), (f, max(int(T) - L // 2, 0)), (f, int(T))]
    return [c[0] for c in crops], [c[1] for c in crops]


def test_features_of_crops_are_the_spectrogram_of_the_crops(paths):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import stft

    for tag, kw, rate, skw in (("native, two channels", {}, 44100, {}),
                               ("16 kHz", dict(sample_rate=16000), 16000, dict(filterbank=None, power=1)),
                               ("16 kHz mono", dict(sample_rate=16000, mono=True), 16000, dict(log="ln")),
                               ("16 kHz mono, complex", dict(sample_rate=16000, mono=True), 16000, dict(filterbank=None, power=None))):
        spec = the_spec(pkg, rate, **skw)
        with pkg.Corpus(paths) as corpus:
            totals = corpus.num_frames if not kw.get("sample_rate") else corpus.resampled_frames(kw["sample_rate"])
            cf, co = the_crops(totals)
            pcm, lengths = corpus.crops(cf, co, L, **kw)
            want, wlen = pkg.spectrogram(pcm, spec, lengths)
            feats, flen = corpus.crops(cf, co, L, features=spec, **kw)
            Co = 1 if kw.get("mono") else corpus.channels
            assert feats.shape == (len(cf), Co, spec.n_mels, 1 + L // 160) and feats.dtype == torch.float32 and feats.is_cuda, tag
            assert same(feats, want), tag
            assert torch.isfinite(feats).all(), tag
            lens = lengths.tolist()
            assert flen.dtype == torch.int64 and flen.tolist() == [n // 160 + 1 for n in lens] == wlen.tolist(), tag
            assert lens[3] == 0
            if spec.log is None:
                assert not feats[3].any(), tag                               # the crop at the file's end is silence
            if spec.power is None:
                z = stft.as_complex(feats)
                assert z.shape == (len(cf), Co, 257, 1 + L // 160) and z.dtype == torch.complex64
            # a crop outside the corpus: feat_lengths -1
            d_f = torch.tensor(cf[:4] + [len(paths)], device="cuda")
            d_o = torch.tensor(co[:4] + [0], device="cuda")
            f2, l2 = corpus.crops(d_f, d_o, L, features=spec, check=False, **kw)
            assert l2.tolist() == flen.tolist()[:4] + [-1] and torch.equal(f2[:4], feats[:4]), tag
            if tag == "16 kHz mono":
                g = torch.Generator(device="cuda")
                g.manual_seed(7)
                r, rl, files, offs = corpus.random_crops(6, L, generator=g, check=False, features=spec, **kw)
                assert r.shape == (6, 1, 24, 1 + L // 160)
                assert torch.equal(r, pkg.spectrogram(corpus.crops(files, offs, L, **kw)[0], spec))


def test_the_stages_behind_it_compose_as_behind_a_logmel(paths):
    import torch

    import alac.net_amd as pkg

    kw = dict(sample_rate=16000, mono=True)
    spec, logspec = the_spec(pkg, 16000), the_spec(pkg, 16000, log="log10")
    with pkg.Corpus(paths) as corpus:
        cf, co = the_crops(corpus.resampled_frames(16000))
        feats, flen = corpus.crops(cf, co, L, features=spec, **kw)
        feats = feats.clone()
        d = pkg.Deltas(2, 2)
        got, l2 = corpus.crops(cf, co, L, features=spec, deltas=d, **kw)
        assert got.shape == (len(cf), 1, 72, feats.shape[-1]) and torch.equal(l2, flen)
        assert same(got, pkg.add_deltas(feats, d, flen)) and torch.equal(got[:, :, :24], feats)
        got, _ = corpus.crops(cf, co, L, features=spec, normalize=pkg.MeanVar(), **kw)
        assert same(got, pkg.normalize(feats, pkg.MeanVar(), flen))
        lf = corpus.crops(cf, co, L, features=logspec, **kw)[0].clone()
        got, _ = corpus.crops(cf, co, L, features=logspec, normalize=pkg.TopDb(80.0), **kw)
        assert same(got, pkg.normalize(lf, pkg.TopDb(80.0), flen))
        pc = pkg.Pcen.like(spec)
        got, _ = corpus.crops(cf, co, L, features=spec, normalize=pc, **kw)
        assert same(got, pkg.normalize(feats, pc, flen)) and not torch.equal(got, feats)
        aug = pkg.SpecAugment(freq_masks=1, freq_width=5, time_masks=1, time_width=4)
        draws = aug.draw(24, flen, generator=torch.Generator(device="cuda").manual_seed(3))
        got, _ = corpus.crops(cf, co, L, features=spec, augment=(aug, draws), **kw)
        assert same(got, pkg.spec_augment(feats, (aug, draws), flen)) and not torch.equal(got, feats)
        # f0= on the frames of the features
        y = pkg.Yin.like(spec, fmin=100.0, fmax=400.0)
        got, l3, track = corpus.crops(cf, co, L, features=spec, f0=y, **kw)
        track = track.clone()
        assert torch.equal(got, feats) and track.shape == (len(cf), 1, 2, feats.shape[-1])
        pcm, lengths = corpus.crops(cf, co, L, **kw)
        assert same(track, pkg.yin(pcm, y, lengths))
        assert pkg.PYin.like(spec).hop_length == 160


def test_refusals_come_before_any_device_work(paths):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(paths) as corpus:
        corpus.crops([0], [0], 500)
        last = corpus._last
        s16, s44 = the_spec(pkg, 16000), the_spec(pkg, 44100)
        z44 = the_spec(pkg, 44100, filterbank=None, power=None)
        aug = pkg.SpecAugment(freq_masks=1, freq_width=5)
        for kw in (dict(features=s16), dict(features=s44, sample_rate=16000), dict(features=s16, sample_rate=22050),
                   dict(features=s44, dtype=torch.int32), dict(features=s44, num_frames=256), dict(features=s44, num_frames=0),
                   dict(features=z44, deltas=pkg.Deltas(2, 2)), dict(features=z44, normalize=pkg.MeanVar()),
                   dict(features=z44, normalize=pkg.Pcen.like(z44)), dict(features=z44, vad=pkg.EnergyVad()), dict(features=z44, augment=aug),
                   dict(features=the_spec(pkg, 44100, log="ln"), normalize=pkg.Pcen.like(s44))):
            n = kw.pop("num_frames", 1000)
            with pytest.raises(ValueError):
                corpus.crops([0], [0], n, **kw)
            with pytest.raises(ValueError):
                corpus.random_crops(2, n, **kw)
        with pytest.raises(ValueError, match="features must be a features.LogMel or a fbank.KaldiFbank"):
            corpus.crops([0], [0], 1000, features="mel")
        assert corpus._last == last and corpus._ft_scratch is None
        got, n1 = corpus.crops([0], [0], 257, features=z44)        # the shortest crop: one frame reflecting at both ends, and one more
        assert got.shape == (1, corpus.channels, 514, 2)
        empty, n0 = corpus.crops([], [], 1000, features=s44)
        assert empty.shape == (0, corpus.channels, 24, 7) and n0.shape == (0,)
