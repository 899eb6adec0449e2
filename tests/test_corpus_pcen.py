"""Corpus.crops(features=LogMel(log=None), normalize=Pcen) on the GPU, on a small synthetic corpus built as
tests/test_corpus_vad.py builds its own: the result is bit for bit `normalize` applied to what the same call returns without
it -- alone, behind vad=, in front of augment=, on the host tier, from files of different rates and through random_crops --,
and the refusals come before any device work.  What the kernel computes is tests/test_pcen.py's subject."""
import numpy as np
import pytest

from test_corpus_vad import FILES, RATE, VAD, same_bits, stretches

pytestmark = pytest.mark.gpu

L = 16000


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    import torch

    import alac.net_amd as pkg

    d = tmp_path_factory.mktemp("corpus_pcen")
    out = []
    for i, (frames, bits, fl, seed) in enumerate(FILES):
        out.append(str(d / f"pcen{i}.m4a"))
        pkg.save(out[-1], stretches(torch, frames, seed), RATE if i else 22050, sample_size=bits, frame_length=fl)
    same = str(d / "pcen0_16k.m4a")
    pkg.save(same, stretches(torch, FILES[0][0], FILES[0][3]), RATE, sample_size=FILES[0][1], frame_length=FILES[0][2])
    return dict(same=[same] + out[1:], mixed=out)


def device_crops(torch, corpus, mixed=False):
    """tests/test_corpus_vad.py's crops, in frames at RATE: per file its first frames, a middle and a crop that runs off the
    end; the last crop is outside the corpus"""
    cf, co = [], []
    for f, T in enumerate(corpus.resampled_frames(RATE) if mixed else corpus.num_frames):
        cf += [f, f, f]
        co += [0, int(T) // 3, int(T) - L // 2]
    return torch.tensor(cf + [corpus.num_files], device="cuda"), torch.tensor(co + [0], device="cuda")


@pytest.mark.parametrize("tier", ["resident", "host", "mixed rates"])
def test_crops_are_normalize_behind_the_same_call_without_it(paths, tier):
    import torch

    import alac.net_amd as pkg

    spec = pkg.LogMel(RATE, n_mels=40, log=None)
    per_bin = pkg.Pcen.like(spec, gain=np.linspace(0.98, 0.6, 40).tolist(), bias=np.linspace(2.0, 0.5, 40).tolist())
    policy = pkg.SpecAugment(freq_masks=1, freq_width=5, time_masks=1, time_width=10)
    made = dict(resident=(paths["same"], {}), host=(paths["same"], dict(hbm_bytes=0)), **{"mixed rates": (paths["mixed"], dict(mixed_rates=True))})[tier]
    with pkg.Corpus(made[0], **made[1]) as corpus:
        d_f, d_o = device_crops(torch, corpus, mixed=tier == "mixed rates")
        for mono, how in ((True, pkg.Pcen.like(spec)), (False, per_bin)):
            kw = dict(sample_rate=RATE, mono=mono, features=spec, check=False)
            base, blen = corpus.crops(d_f, d_o, L, **kw)
            base = base.clone()
            want = pkg.normalize(base, how, blen)
            got, glen = corpus.crops(d_f, d_o, L, normalize=how, **kw)
            assert same_bits(torch, got, want) and torch.equal(glen, blen), (tier, mono)
            assert blen[-1] == -1 and (got[-1] == 0).all() and torch.isfinite(got).all()
            assert not same_bits(torch, got, base)
            # into `out`
            out = torch.full_like(base, float("nan"))
            res = corpus.crops(d_f, d_o, L, normalize=how, out=out, **kw)
            assert res[0] is out and same_bits(torch, out, want)
            # behind vad=: the decision on the energies, the compression over all frames, then the selection
            vad = pkg.EnergyVad(**VAD)
            mask = pkg.vad_energy(base, vad, blen)
            sel, new = pkg.select_frames(want, mask, blen)
            got_v, len_v = corpus.crops(d_f, d_o, L, vad=vad, normalize=how, **kw)
            assert same_bits(torch, got_v, sel) and torch.equal(len_v, new)
            # in front of augment=
            draws = policy.draw(base.shape[2], blen)
            got_a, len_a = corpus.crops(d_f, d_o, L, normalize=how, augment=(policy, draws), **kw)
            assert same_bits(torch, got_a, pkg.spec_augment(want, (policy, draws), blen)) and torch.equal(len_a, blen)


def test_the_kaldi_fbank_energies_and_constant_q_take_it_too(paths):
    import torch

    import alac.net_amd as pkg

    with pkg.Corpus(paths["same"]) as corpus:
        d_f, d_o = device_crops(torch, corpus)
        for spec in (pkg.KaldiFbank(RATE, n_mels=23, log=False), pkg.ConstantQ(RATE, hop_length=256, f_min=110.0, n_bins=24, log=None)):
            how = pkg.Pcen.like(spec, time_constant=0.06)
            kw = dict(mono=True, features=spec, check=False)
            base, blen = corpus.crops(d_f, d_o, L, **kw)
            want = pkg.normalize(base.clone(), how, blen)
            got, glen = corpus.crops(d_f, d_o, L, normalize=how, **kw)
            assert same_bits(torch, got, want) and torch.equal(glen, blen), spec


def test_random_crops_reproduce(paths):
    import torch

    import alac.net_amd as pkg

    spec = pkg.LogMel(RATE, log=None)
    how = pkg.Pcen.like(spec)
    with pkg.Corpus(paths["same"]) as corpus:
        kw = dict(sample_rate=RATE, mono=True, features=spec, check=False)
        a = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(11), normalize=how, **kw)
        b = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(11), normalize=how, **kw)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert a[0].shape == (6, 1, 80, spec.frames(L)) and a[1].dtype == torch.int64 and a[1].is_cuda
        plain = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(11), **kw)
        assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3]) and torch.equal(plain[1], a[1])
        assert same_bits(torch, a[0], pkg.normalize(plain[0].clone(), how, plain[1]))
        # the README's step
        res = corpus.random_crops(8, 32000, sample_rate=16000, mono=True, features=spec, normalize=how, check=False)
        assert res[0].shape == (8, 1, 80, 201) and torch.isfinite(res[0]).all()


def test_corpus_refuses_before_any_device_work(paths):
    import torch

    import alac.net_amd as pkg

    energy = pkg.LogMel(RATE, n_mels=40, log=None)
    how = pkg.Pcen.like(energy)
    with pkg.Corpus(paths["same"]) as corpus:
        for kw in (dict(normalize=how),                                                        # no features=
                   dict(normalize=how, features=pkg.LogMel(RATE)), dict(normalize=how, features=pkg.LogMel(RATE, log="log10")),
                   dict(normalize=how, features=pkg.ConstantQ(RATE, log="log10")), dict(normalize=how, features=pkg.KaldiFbank(RATE)),
                   dict(normalize=how, features=pkg.KaldiMfcc(RATE)),
                   dict(normalize=how, features=energy, deltas=pkg.Deltas(1, 2)),
                   dict(normalize=pkg.Pcen(0.1, gain=[0.9] * 39), features=energy),
                   dict(normalize=pkg.Pcen(0.1, gain=[0.9] * 41), features=energy, mono=True)):
            with pytest.raises(ValueError):
                corpus.crops([0], [0], L, **kw)
        with pytest.raises(ValueError):
            corpus.random_crops(2, L, normalize=how)
        assert corpus.crops([0], [0], L, features=energy, normalize=pkg.Pcen(0.1, gain=[0.9] * 40))[0].shape[2] == 40
