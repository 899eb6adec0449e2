"""Corpus.crops(features=spec) on the GPU: the features of a crop are `log_mel` of that crop bit for bit (the same kernel on the
same data: crops(features=) only saves the caller the PCM tensor), on every path a crop can take -- the corpus's own rate,
another rate as mono, files of different rates, and a corpus tiered between HBM and host memory; the feature lengths, `out=`,
`check=False`, the refusals, and random crops.  What the kernel computes is tests/test_features.py's subject."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
# (sample rate, frames, bits, frame length)
SAME = [(44100, 20000, 16, 4096), (44100, 9001, 24, 1024), (44100, 12000, 16, 1024)]
MIXED = [(44100, 20000, 16, 4096), (48000, 18001, 24, 1024), (16000, 12000, 16, 1024)]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    d = tmp_path_factory.mktemp("corpus_features")
    out = {}
    for name, spec in (("same", SAME), ("mixed", MIXED)):
        out[name] = []
        for i, (rate, frames, bits, fl) in enumerate(spec):
            path = str(d / f"{name}{i}_{rate}.m4a")
            pkg.save(path, signal(torch, rate, frames, 70 + i), rate, sample_size=bits, frame_length=fl)
            out[name].append(path)
    return out


def the_crops(totals):
    """Per file: its first frames, a middle, a crop that runs off the end, and the crop at the very end (length 0)"""
    crops = []
    for f, T in enumerate(totals):
        crops += [(f, 0), (f, int(T) // 3), (f, max(int(T) - L // 2, 0)), (f, int(T))]
    return [c[0] for c in crops], [c[1] for c in crops]


def corpora(pkg, paths):
    """(tag, corpus arguments, crops arguments, the rate of the crops)"""
    import os

    some = sum(os.path.getsize(p) for p in paths["same"][:1])
    return [("native", (paths["same"], {}), {}, 44100),
            ("16 kHz mono", (paths["same"], {}), dict(sample_rate=16000, mono=True), 16000),
            ("mixed rates", (paths["mixed"], dict(mixed_rates=True)), dict(sample_rate=16000), 16000),
            ("mixed rates mono", (paths["mixed"], dict(mixed_rates=True)), dict(sample_rate=16000, mono=True), 16000),
            ("host tier", (paths["same"], dict(hbm_bytes=0)), {}, 44100),
            ("two tiers, 16 kHz", (paths["same"], dict(hbm_bytes=some)), dict(sample_rate=16000), 16000)]


def test_features_of_crops_are_log_mel_of_the_crops(paths):
    import torch

    import alac.net_amd as pkg

    for tag, (src, ckw), kw, rate in corpora(pkg, paths):
        spec = pkg.LogMel(rate, 400, 160, 80)
        with pkg.Corpus(src, **ckw) as corpus:
            totals = corpus.num_frames if not kw.get("sample_rate") else corpus.resampled_frames(kw["sample_rate"])
            cf, co = the_crops(totals)
            pcm, lengths = corpus.crops(cf, co, L, **kw)
            want = pkg.log_mel(pcm, spec)
            feats, flen = corpus.crops(cf, co, L, features=spec, **kw)
            Co = 1 if kw.get("mono") else corpus.channels
            assert feats.shape == (len(cf), Co, 80, 1 + L // 160) and feats.dtype == torch.float32 and feats.is_cuda, tag
            assert torch.equal(feats.view(torch.int32), want.view(torch.int32)), tag
            assert torch.isfinite(feats).all(), tag
            lens = lengths.tolist()
            assert lens == [min(L, int(totals[f]) - o) for f, o in zip(cf, co)], tag
            assert flen.dtype == torch.int64 and flen.is_cuda and flen.tolist() == [n // 160 + 1 for n in lens], tag
            # the crop at the file's end is silence: log(floor) everywhere
            assert lens[3] == 0 and (feats[3] == feats[3].flatten()[0]).all() and abs(float(feats[3].flatten()[0]) - np.log(1e-10)) < 1e-4
            # indices on the device, one of them outside the corpus and one offset behind its file: -1 and a row of silence
            d_f = torch.tensor(cf[:4] + [len(src), 0], device="cuda")
            d_o = torch.tensor(co[:4] + [0, int(totals[0]) + 1], device="cuda")
            f2, l2 = corpus.crops(d_f, d_o, L, features=spec, check=False, **kw)
            assert l2.tolist() == flen.tolist()[:4] + [-1, -1], tag
            assert torch.equal(f2[:4], feats[:4]) and (f2[4:] == feats[3].flatten()[0]).all(), tag
            with pytest.raises(ValueError):
                corpus.crops(d_f, d_o, L, features=spec, **kw)          # check=True names the crop with the negative length
            print(f"{tag}: {len(cf)} crops, lengths {lens}")


def test_out_unchecked_calls_and_the_scratch(paths):
    import torch

    import alac.net_amd as pkg

    spec = pkg.LogMel(16000, 400, 160, 80, log="log10")
    with pkg.Corpus(paths["same"]) as corpus:
        Ty = corpus.resampled_frames(16000)
        cf, co = the_crops(Ty)
        kw = dict(sample_rate=16000, mono=True)
        feats, flen = corpus.crops(cf, co, L, features=spec, **kw)
        out = torch.full_like(feats, float("nan"))
        got, flen2 = corpus.crops(cf, co, L, features=spec, out=out, check=False, **kw)
        assert got is out and torch.equal(out, feats) and torch.equal(flen, flen2)
        status, mask = corpus.last_status()
        assert int(mask.sum()) > 0 and not status[mask].any()
        scratch = corpus._ft_scratch
        corpus.crops(cf[:3], co[:3], L, features=spec, **kw)
        assert corpus._ft_scratch is scratch                     # kept, and grown only when a call needs more
        corpus.crops(cf, co, 2 * L, features=spec, **kw)
        assert corpus._ft_scratch.numel() >= len(cf) * 2 * L
        # the PCM path is what it was
        pcm, lengths = corpus.crops(cf, co, L, **kw)
        assert pcm.shape == (len(cf), 1, L) and torch.equal(pkg.log_mel(pcm, spec), feats)
        for bad in (torch.empty((len(cf), 1, 80, 1 + L // 160), dtype=torch.float64, device="cuda"),
                    torch.empty((len(cf), 1, 80, L // 160), device="cuda"), torch.empty((len(cf), 1, 80, 1 + L // 160)),
                    torch.empty((len(cf), 1, 1 + L // 160, 80), device="cuda").transpose(2, 3)):
            with pytest.raises(ValueError, match="out must be"):
                corpus.crops(cf, co, L, features=spec, out=bad, **kw)


def test_refusals_come_before_any_device_work(paths):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(paths["same"]) as corpus, pkg.Corpus(paths["mixed"], mixed_rates=True) as mixed:
        corpus.crops([0], [0], 500)
        last = corpus._last
        s16, s44 = pkg.LogMel(16000), pkg.LogMel(44100)
        for kw in (dict(features=s16), dict(features=s44, sample_rate=16000), dict(features=s16, sample_rate=22050),
                   dict(features=s44, dtype=torch.int32), dict(features=s44, dtype="int32"), dict(features="log-mel"),
                   dict(features=s44, num_frames=200), dict(features=s44, num_frames=0)):
            n = kw.pop("num_frames", 1000)
            with pytest.raises(ValueError):
                corpus.crops([0], [0], n, **kw)
            with pytest.raises(ValueError):
                corpus.random_crops(2, n, **kw)
        with pytest.raises(ValueError, match="LogMel"):
            corpus.crops([0], [0], 1000, None, None, True, 16000)     # a rate where the features go
        assert corpus._last == last and corpus._ft_scratch is None
        corpus.crops([0], [0], 201, features=s44)                 # the shortest crop
        corpus.crops([0], [0], 1000, features=s44, dtype=torch.float32)
        with pytest.raises(ValueError, match="sample_rate="):
            mixed.crops([0], [0], 1000, features=s16)
        with pytest.raises(ValueError):
            mixed.crops([0], [0], 1000, features=s44, sample_rate=16000)
        empty, n0 = corpus.crops([], [], 1000, features=s44)
        assert empty.shape == (0, corpus.channels, 80, 7) and n0.shape == (0,)


def test_random_crops_with_a_generator_are_reproducible(paths):
    import torch

    import alac.net_amd as pkg

    spec = pkg.LogMel(16000, 400, 160, 40)
    with pkg.Corpus(paths["mixed"], mixed_rates=True) as corpus:
        runs = []
        for _ in range(2):
            g = torch.Generator(device="cuda")
            g.manual_seed(1234)
            runs.append(corpus.random_crops(16, L, generator=g, sample_rate=16000, mono=True, features=spec))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        feats, flen, files, offs = runs[0]
        assert feats.shape == (16, 1, 40, 1 + L // 160) and flen.tolist() == [1 + L // 160] * 16
        pcm = corpus.crops(files, offs, L, sample_rate=16000, mono=True)[0]
        assert torch.equal(pkg.log_mel(pcm, spec), feats)
