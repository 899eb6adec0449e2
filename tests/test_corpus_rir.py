"""Corpus.crops(reverb=) and Corpus.random_crops(reverb=) with a Reverb over simulated rooms, on the GPU: the crops are held bit
for bit to alac.reverb of the crops without reverb= and alac.simulate_rir of the draws; p = 0 to the crops themselves; the
draws to a seed; the stage composes with mix= and features=; and a Reverb over a corpus of responses with given draws gives
what it gave."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 3000
RATE = 16000
SECONDS = 0.04                    # 640 frames at 16 kHz: ten tiles, a few thousand images a room


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpora(synth, tmp_path_factory):
    import torch

    import alac.net_amd as pkg
    from test_load_window import make_file

    sig = [make_file(synth, n, last, ss, True, seed=260 + i)[0] for i, (n, last, ss) in enumerate([(3, 100, 16), (2, 4000, 24)])]
    noise = [make_file(synth, 2, 2000, 16, False, seed=280)[0]]
    d = tmp_path_factory.mktemp("rirs")
    rng = np.random.default_rng(9)
    h = 0.3 * rng.standard_normal((1, 900)) * np.exp(-np.arange(900) / 150.0)
    h[:, 10] = 0.9
    path = str(d / "m0.m4a")
    pkg.save(path, torch.from_numpy(h.astype(np.float32)).cuda(), 44100, frame_length=1024)
    with pkg.Corpus(sig) as c, pkg.Corpus(noise) as n, pkg.Corpus([path]) as r:
        yield dict(sig=c, noise=n, rirs=r)


def rooms_and_draws(pkg, torch, p=0.7):
    rooms = pkg.ShoeboxRooms(room=((3, 5), (3, 4), (2.5, 3)), absorption=(0.3, 0.6))
    aug = pkg.Reverb(rooms, p=p, max_seconds=SECONDS)
    geometry, beta, _ = aug.draw(4, generator=torch.Generator(device="cuda").manual_seed(3), device=torch.device("cuda", 0))
    geometry[2, 3] = geometry[2, 0] + 1.0                          # a source outside its room: that row is refused
    keep = torch.tensor([True, False, True, True], device="cuda")
    return aug, (geometry, beta, keep)


def crops_of(torch, corpus):
    return torch.tensor([0, 1, 1, 0], device="cuda"), torch.tensor([0, 500, 17, 2500], device="cuda")


def test_crops_with_rooms_are_reverb_of_the_crops_and_the_simulated_responses(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    aug, draws = rooms_and_draws(pkg, torch)
    cf, co = crops_of(torch, corpus)
    kw = dict(sample_rate=RATE, mono=True, check=False)
    pcm, lengths = corpus.crops(cf, co, L, **kw)
    pcm = pcm.clone()
    K = aug.frames(RATE)
    h, hlen = pkg.simulate_rir(draws[0], draws[1], RATE, K)
    assert K == 640 and hlen.cpu().tolist() == [K, K, 0, K]
    want = pkg.reverb(pcm, h, lengths, torch.where(draws[2], hlen, 0))
    got, glen = corpus.crops(cf, co, L, reverb=(aug, draws), **kw)
    assert torch.equal(glen, lengths) and torch.equal(bits(got), bits(want))
    assert torch.equal(bits(got[1]), bits(pcm[1])) and torch.equal(bits(got[2]), bits(pcm[2]))       # not kept; refused
    assert not torch.equal(bits(got[0]), bits(pcm[0])) and not torch.equal(bits(got[3]), bits(pcm[3]))
    for bad in ((draws[0], draws[1]), (draws[0].float(), draws[1], draws[2]), (draws[0], draws[1], draws[2].long()),
                (draws[0].cpu(), draws[1].cpu(), draws[2].cpu()), (draws[0][:3], draws[1][:3], draws[2][:3])):
        with pytest.raises(ValueError):
            corpus.crops(cf, co, L, reverb=(aug, bad), **kw)
    with pytest.raises(ValueError):
        corpus.crops(cf, co, L, reverb=aug, dtype=torch.int32, sample_rate=RATE, mono=True)


def test_random_crops_are_reproducible_and_p_0_changes_nothing(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    aug, _ = rooms_and_draws(pkg, torch)

    def run(**kw):
        g = torch.Generator(device="cuda").manual_seed(11)
        out = corpus.random_crops(5, L, sample_rate=RATE, mono=True, generator=g, **kw)
        return out[0].clone(), out[1].clone()

    a, b, plain = run(reverb=aug), run(reverb=aug), run()
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])
    assert not torch.equal(bits(a[0]), bits(plain[0]))
    none = run(reverb=pkg.Reverb(aug.rirs, p=0.0, max_seconds=SECONDS))
    assert torch.equal(bits(none[0]), bits(plain[0])) and torch.equal(none[1], plain[1])


def test_rooms_compose_with_mix_and_features(corpora):
    import torch

    import alac.net_amd as pkg

    corpus = corpora["sig"]
    aug, draws = rooms_and_draws(pkg, torch)
    cf, co = crops_of(torch, corpus)
    kw = dict(sample_rate=RATE, mono=True, check=False)
    noise = pkg.AddNoise(corpora["noise"], snr_db=(5.0, 15.0))
    nd = noise.draw(4, L, sample_rate=RATE, generator=torch.Generator(device="cuda").manual_seed(5))
    spec = pkg.LogMel(RATE, n_fft=400, hop_length=160, n_mels=40)
    wet, lengths = corpus.crops(cf, co, L, reverb=(aug, draws), **kw)
    wet = wet.clone()
    mixed, _ = corpus.crops(cf, co, L, reverb=(aug, draws), mix=(noise, nd), **kw)
    mixed = mixed.clone()
    assert not torch.equal(bits(mixed), bits(wet))
    feats = corpus.crops(cf, co, L, reverb=(aug, draws), mix=(noise, nd), features=spec, **kw)[0]
    assert torch.equal(bits(feats), bits(pkg.log_mel(mixed, spec, lengths)[0]))


def test_a_reverb_over_a_corpus_gives_what_it_gave(corpora):
    import torch

    import alac.net_amd as pkg

    corpus, rirs = corpora["sig"], corpora["rirs"]
    aug = pkg.Reverb(rirs, p=0.7, max_seconds=SECONDS)
    assert aug.rooms is None
    cf, co = crops_of(torch, corpus)
    draws = (torch.zeros(4, dtype=torch.int64, device="cuda"), torch.tensor([True, False, True, True], device="cuda"))
    kw = dict(sample_rate=RATE, mono=True, check=False)
    K = aug.frames(RATE)
    h, hlen = rirs.crops(draws[0], torch.zeros_like(draws[0]), K, sample_rate=RATE, mono=False, check=False)
    h = h.clone()
    pcm, lengths = corpus.crops(cf, co, L, **kw)
    want = pkg.reverb(pcm.clone(), h, lengths, torch.where(draws[1], hlen, 0))
    got, _ = corpus.crops(cf, co, L, reverb=(aug, draws), **kw)
    assert torch.equal(bits(got), bits(want))
    files, keep = aug.draw(64, generator=torch.Generator(device="cuda").manual_seed(1))
    assert files.shape == (64,) and keep.dtype == torch.bool
