"""What the one crop pipeline of Corpus must keep and no other test asserts: a resident corpus from PCM never fetches its
packet tables for a step, whatever the kind of crop; every kind of crop refuses a closed corpus; and the public K and S are
those of the module-level functions, with a source window per file where the rates differ.

And the stages of a step: crops(reverb=, mix=, features=, normalize=) in every combination is, bit for bit, the public tensor
functions composed over the plain crops in the documented order -- alac.reverb, alac.mix, alac.log_mel, alac.normalize --, with
the lengths and last_status() of the plain crops, on the native path and on the sample_rate= / mono= path; and the draws of
random_crops and of crops come from one generator in the documented order, mix before reverb."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, L, TARGET = 4, 1000, 16000
RATES = (44100, 48000)
LENGTHS = [12000, 11111]        # two files of about three packets of 4096 frames


@pytest.fixture(scope="module")
def material():
    """(pcm float32 [2, 2, 12000] on the device, the two files of it as M4A bytes at 44100 Hz, the same two at 44100 and 48000)"""
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    pcm = torch.stack([signal(torch, RATES[0], max(LENGTHS), 70 + f) for f in range(2)])

    def files(rates):
        out = []
        for f, rate in enumerate(rates):
            buf = io.BytesIO()
            pkg.save_batch([buf], pcm[f:f + 1], LENGTHS[f:f + 1], rate)
            out.append(buf.getvalue())
        return out

    return pcm, files((RATES[0], RATES[0])), files(RATES)


def calls(corpus, rate):
    """The four kinds of call, on device indices and unchecked; `rate`: the corpus's own"""
    import torch

    from alac.net_amd.features import LogMel

    files = torch.tensor([0, 1, 1, 0], device="cuda")
    offs = torch.tensor([0, 17, 2500, 3000], device="cuda")
    return {"native": lambda: corpus.crops(files, offs, L, check=False),
            "sample_rate": lambda: corpus.crops(files, offs, L, check=False, sample_rate=TARGET),
            "mono": lambda: corpus.crops(files, offs, L, check=False, mono=True),
            "features": lambda: corpus.crops(files, offs, L, check=False, features=LogMel(rate))}


def test_a_resident_corpus_from_pcm_reads_no_packet_table_for_any_kind_of_crop(material):
    import torch

    import alac.net_amd as pkg

    pcm, _, mixed_files = material
    with pkg.Corpus.from_pcm(pcm, LENGTHS, RATES[0]) as corpus:
        assert corpus.tier_bytes[1] == 0
        for name, call in calls(corpus, RATES[0]).items():
            out, lengths = call()
            assert out.shape[0] == B and (lengths > 0).all(), name
            assert "pkt_size" not in corpus._host and "pkt_offset" not in corpus._host, name
    with pkg.Corpus(mixed_files, mixed_rates=True) as corpus:
        assert corpus.sample_rate is None
        before = set(corpus._host)
        files, offs = torch.tensor([0, 1, 1, 0], device="cuda"), torch.tensor([0, 17, 2500, 3000], device="cuda")
        out, lengths = corpus.crops(files, offs, L, check=False, sample_rate=TARGET)
        assert out.shape == (B, 2, L) and (lengths == L).all()
        assert set(corpus._host) == before


def test_every_kind_of_crop_refuses_a_closed_corpus(material):
    import alac.net_amd as pkg

    pcm, _, mixed_files = material
    corpus = pkg.Corpus.from_pcm(pcm, LENGTHS, RATES[0])
    corpus.close()
    for name, call in calls(corpus, RATES[0]).items():
        with pytest.raises(pkg.AlacGpuError, match="the corpus is closed"):
            call()
    corpus = pkg.Corpus(mixed_files, mixed_rates=True)
    corpus.close()
    with pytest.raises(pkg.AlacGpuError, match="the corpus is closed"):
        corpus.crops([0, 1], [0, 0], L, sample_rate=TARGET)


def test_the_public_bounds_are_the_module_level_functions(material):
    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_table, source_window

    _, same_files, mixed_files = material
    with pkg.Corpus(same_files) as corpus, pkg.Corpus(same_files, hbm_bytes=0) as tiered:
        h = corpus._host
        assert corpus.entries_per_crop(L, sample_rate=TARGET) == corpus.entries_per_crop(L) == \
            max(pkg.entries_per_crop(h["pkt_end"], h["file_first"], L), 1)
        assert tiered.tier_bytes[0] == 0 and tiered.tier_bytes[1] > 0
        assert tiered.stage_bytes_per_crop(L, sample_rate=TARGET) == tiered.stage_bytes_per_crop(L) == \
            pkg.stage_bytes_per_crop(h["pkt_size"], h["pkt_end"], h["file_first"], L) > 0
    with pkg.Corpus(mixed_files, mixed_rates=True) as corpus:
        Ls = np.array([source_window(0, L, *resample_table(rate, TARGET)[:3])[1] for rate in RATES], dtype=np.int64)
        assert Ls[0] != Ls[1]
        h = corpus._host
        assert corpus.entries_per_crop(L, sample_rate=TARGET) == max(pkg.entries_per_crop(h["pkt_end"], h["file_first"], Ls), 1)
        assert corpus.stage_bytes_per_crop(L, sample_rate=TARGET) == \
            pkg.stage_bytes_per_crop(h["pkt_size"], h["pkt_end"], h["file_first"], Ls) > 0


# ---- the stages of a step ------------------------------------------------------------------------------------------------------
SL = 2500                       # more than one reverb hop of 2048 and more than n_fft // 2
RIR_FRAMES = 2100               # at the rate of the crops: two partitions of 2048
SIG_RATE = 48000
STAGES = ("reverb", "mix", "features", "normalize")
PATHS = {"native": dict(), "rate": dict(sample_rate=TARGET, mono=True), "rate_self_noise": dict(sample_rate=TARGET, mono=True)}


def saved(pkg, torch, x, rate):
    buf = io.BytesIO()
    pkg.save(buf, x, rate)
    return buf.getvalue()


@pytest.fixture(scope="module")
def staged():
    """The signal (three stereo files at 48 kHz), a noise corpus (one channel at 22.05 kHz, one file shorter than a crop) and
    a corpus of impulse responses (two channels at 44.1 kHz: decaying noise, one file shorter than RIR_FRAMES at either rate
    of the crops, one longer)"""
    import torch

    import alac.net_amd as pkg
    from test_corpus_mixed_rates import signal

    rng = np.random.default_rng(23)
    sig = [saved(pkg, torch, signal(torch, SIG_RATE, n, 200 + i), SIG_RATE) for i, n in enumerate([30000, 24000, 9000])]
    noise = [saved(pkg, torch, torch.from_numpy((0.1 * rng.standard_normal((1, n))).astype(np.float32)).cuda(), 22050)
             for n in (9000, 1000)]

    def response(frames):
        h = 0.3 * rng.standard_normal((2, frames)) * np.exp(-np.arange(frames) / (frames / 6.0))
        h[:, [10, 13]] = 0.9                                                      # the direct path
        return saved(pkg, torch, torch.from_numpy(h.astype(np.float32)).cuda(), 44100)

    with pkg.Corpus(sig) as c, pkg.Corpus(noise) as n, pkg.Corpus([response(7000), response(1500)]) as r:
        assert (c.channels, n.channels, r.channels) == (2, 1, 2) and (c.sample_rate, n.sample_rate, r.sample_rate) == (SIG_RATE, 22050, 44100)
        yield dict(sig=c, noise=n, rirs=r)


def stage_batch(torch, corpus, totals):
    """Six crops as device tensors -- the third runs past its file's end, the fourth names a file outside the corpus -- and
    their draws: the fifth keeps no response, the sixth draws NaN for its ratio"""
    cf = torch.tensor([0, 1, 2, corpus.num_files, 1, 0], device="cuda")
    co = torch.tensor([0, int(totals[1]) // 3, int(totals[2]) - SL // 2, 0, 100, 17], device="cuda")
    ndraws = (torch.tensor([0, 1, 0, 1, 1, 0], device="cuda"), torch.tensor([0, 0, 300, 100, 50, 1000], device="cuda"),
              torch.tensor([10.0, 5.0, 0.0, 15.0, 20.0, float("nan")], device="cuda"))
    rdraws = (torch.tensor([0, 1, 0, 1, 0, 1], device="cuda"), torch.tensor([True, True, True, True, False, True], device="cuda"))
    return cf, co, ndraws, rdraws


def composed(pkg, torch, x, lengths, h, hlen, n, nlen, ndraws, rdraws, spec, on):
    """The public tensor functions over clones of the plain crops x, in the documented order; `on`: stage -> its argument"""
    y, lens = x.clone(), lengths
    if "reverb" in on:
        y = pkg.reverb(y, h, lengths, torch.where(rdraws[1], hlen, 0))
    if "mix" in on:
        y = pkg.mix(y, n, ndraws[2], lengths, nlen)
    if "features" in on:
        y, lens = pkg.log_mel(y, spec, lengths)
    if "normalize" in on:
        y = pkg.normalize(y, on["normalize"], lens)
    return y, lens


@pytest.mark.parametrize("path", list(PATHS))
def test_every_combination_of_stages_is_the_public_functions_composed_over_the_plain_crops(staged, path):
    import itertools

    import torch

    import alac.net_amd as pkg

    kw = PATHS[path]
    corpus, rirs = staged["sig"], staged["rirs"]
    noise = corpus if path == "rate_self_noise" else staged["noise"]
    rate = kw.get("sample_rate") or corpus.sample_rate
    Co = 1 if kw.get("mono") else corpus.channels
    cf, co, ndraws, rdraws = stage_batch(torch, corpus, corpus.resampled_frames(rate) if kw else corpus.num_frames)
    add, aug = pkg.AddNoise(noise, (0, 20)), pkg.Reverb(rirs, max_seconds=RIR_FRAMES / rate)
    spec = pkg.LogMel(rate, 400, 160, 80)
    assert aug.frames(rate) == RIR_FRAMES
    # the companions by the second corpora's own crops, then the plain crops and their statuses
    n, nlen = noise.crops(ndraws[0], ndraws[1], SL, sample_rate=rate, mono=noise.channels != Co, check=False)
    n = n.clone()
    h, hlen = rirs.crops(rdraws[0], torch.zeros_like(rdraws[0]), RIR_FRAMES, sample_rate=rate, mono=rirs.channels != Co, check=False)
    h = h.clone()
    x, lengths = corpus.crops(cf, co, SL, check=False, **kw)
    x = x.clone()
    status = tuple(t.clone() for t in corpus.last_status())
    ll = lengths.tolist()
    assert x.shape == (6, Co, SL) and ll[3] == -1 and 0 < ll[2] < SL and ll[:2] + ll[4:] == [SL] * 4
    assert h.shape == (6, Co, RIR_FRAMES) and (hlen == RIR_FRAMES).any() and (hlen < RIR_FRAMES).any()
    assert n.shape == (6, 1, SL) and ((nlen < SL).any() or noise is corpus)
    subsets = [c for k in range(len(STAGES) + 1) for c in itertools.combinations(STAGES, k)]
    assert len(subsets) == 16
    for names in subsets:
        if path == "rate_self_noise" and "mix" not in names:
            continue
        hows = [pkg.MeanVar(eps=1e-5)] + ([pkg.TopDb.whisper()] if "features" in names else []) if "normalize" in names else [None]
        for how in hows:
            on = dict(reverb=(aug, rdraws), mix=(add, ndraws), features=spec, normalize=how)
            on = {k: on[k] for k in names}
            want, want_len = composed(pkg, torch, x, lengths, h, hlen, n, nlen, ndraws, rdraws, spec, on)
            got, got_len = corpus.crops(cf, co, SL, check=False, **on, **kw)
            assert got.shape == want.shape and torch.equal(got, want), (names, how)
            assert got_len.dtype == torch.int64 and torch.equal(got_len, want_len), (names, how)
            assert all(torch.equal(a, b) for a, b in zip(corpus.last_status(), status)), (names, how)
            if names and "features" not in names:
                assert not torch.equal(got, x), names
            if "reverb" in names and "mix" not in names and "features" not in names and how is None:
                assert torch.equal(got[4], x[4]) and not torch.equal(got[5], x[5])               # keep False; a NaN ratio is mix's
            if names == ("mix",):
                assert torch.equal(got[5], x[5]) and torch.equal(got[3], x[3]) and not torch.equal(got[4], x[4])


@pytest.mark.parametrize("path", ["native", "rate"])
def test_the_draws_of_a_step_come_in_the_documented_order(staged, path):
    import torch

    import alac.net_amd as pkg

    kw = PATHS[path]
    corpus = staged["sig"]
    rate = kw.get("sample_rate") or corpus.sample_rate
    add, aug = pkg.AddNoise(staged["noise"], (0, 20), p=0.8), pkg.Reverb(staged["rirs"], p=0.8, max_seconds=RIR_FRAMES / rate)
    stages = dict(features=pkg.LogMel(rate, 400, 160, 80), normalize=pkg.MeanVar(eps=1e-5))
    a = corpus.random_crops(6, SL, generator=torch.Generator(device="cuda").manual_seed(5), mix=add, reverb=aug, check=False, **stages, **kw)
    b = corpus.random_crops(6, SL, generator=torch.Generator(device="cuda").manual_seed(5), mix=add, reverb=aug, check=False, **stages, **kw)
    assert len(a) == 4 and all(torch.equal(s, t) for s, t in zip(a, b))
    # the call's own two draws, then AddNoise.draw's four, then Reverb.draw's two, from one generator
    g = torch.Generator(device="cuda").manual_seed(5)
    plain = corpus.random_crops(6, SL, generator=g, check=False, **kw)
    ndraws = add.draw(6, SL, sample_rate=rate, generator=g)
    rdraws = aug.draw(6, generator=g)
    assert torch.equal(plain[2], a[2]) and torch.equal(plain[3], a[3])
    again = corpus.crops(a[2], a[3], SL, mix=(add, ndraws), reverb=(aug, rdraws), check=False, **stages, **kw)
    assert torch.equal(again[0], a[0]) and torch.equal(again[1], a[1])
    swapped = corpus.crops(a[2], a[3], SL, mix=(add, ndraws), reverb=(aug, aug.draw(6, generator=g)), check=False, **stages, **kw)
    assert not torch.equal(swapped[0], a[0])
    # crops without draws makes them from the device's default generator in the same order
    torch.cuda.manual_seed(9)
    drawn = corpus.crops(a[2], a[3], SL, mix=add, reverb=aug, check=False, **stages, **kw)[0].clone()
    torch.cuda.manual_seed(9)
    ndraws = add.draw(6, SL, sample_rate=rate)
    rdraws = aug.draw(6)
    assert torch.equal(corpus.crops(a[2], a[3], SL, mix=(add, ndraws), reverb=(aug, rdraws), check=False, **stages, **kw)[0], drawn)


def test_all_six_drawing_stages_draw_in_the_documented_order(staged):
    """speed=, pitch=, mix=, reverb=, effects= and augment= at once, with features= and deltas=: random_crops draws files, u,
    speed, pitch, mix, reverb, effects, augment from its generator; crops draws pitch, mix, reverb, effects, speed, augment
    from the device's default generator -- the SpeedPerturb behind the Effects"""
    import torch

    import alac.net_amd as pkg

    kw = PATHS["rate"]
    corpus, rate, dev = staged["sig"], TARGET, torch.device("cuda", 0)
    sp, ps = pkg.SpeedPerturb(), pkg.PitchShift()
    add, aug = pkg.AddNoise(staged["noise"], (0, 20), p=0.8), pkg.Reverb(staged["rirs"], p=0.8, max_seconds=RIR_FRAMES / rate)
    fx = pkg.Effects(pkg.RandomBiquad("peaking", (200.0, 6000.0), q=(0.5, 2.0), gain_db=(-3.0, 0.0)), gain_db=(-3.0, 0.0))
    sa = pkg.SpecAugment(freq_width=10, time_width=5, time_warp=3)
    spec, dl = pkg.LogMel(rate, 400, 160, 80), pkg.Deltas()
    stages = dict(features=spec, deltas=dl)
    lines, frames = dl.lines(spec.n_mels), spec.frames(SL)
    seeded = lambda: torch.Generator(device="cuda").manual_seed(11)
    a = corpus.random_crops(6, SL, generator=seeded(), speed=sp, pitch=ps, mix=add, reverb=aug, effects=fx, augment=sa, check=False,
                            **stages, **kw)
    assert len(a) == 4 and a[0].shape == (6, 1, lines, frames)

    def by_hand(order):
        """The draws of random_crops from an equally seeded generator, the four middle ones in `order`"""
        g = seeded()
        files = torch.randint(0, corpus.num_files, (6,), generator=g, device=dev, dtype=torch.int64)
        u = torch.rand(6, generator=g, device=dev, dtype=torch.float64)
        sdraws = sp.draw(6, generator=g, device=dev)
        ends = torch.from_numpy(corpus.resampled_frames(rate, sp)).to(dev)[files, sdraws]
        span = (ends - SL).clamp(min=0)
        offs = torch.minimum(torch.floor(u * (span + 1).to(torch.float64)).to(torch.int64), span)
        draw = dict(pitch=lambda: ps.draw(6, generator=g, device=dev), mix=lambda: add.draw(6, SL, sample_rate=rate, generator=g),
                    reverb=lambda: aug.draw(6, generator=g, device=dev), effects=lambda: fx.draw(6, rate, generator=g, device=dev))
        drawn = {k: draw[k]() for k in order}
        adraws = sa.draw(lines, spec.lengths((ends - offs).clamp(max=SL)), generator=g)
        return files, offs, corpus.crops(files, offs, SL, speed=(sp, sdraws), pitch=(ps, drawn["pitch"]), mix=(add, drawn["mix"]),
                                         reverb=(aug, drawn["reverb"]), effects=(fx, drawn["effects"]), augment=(sa, adraws),
                                         check=False, **stages, **kw)

    files, offs, again = by_hand(("pitch", "mix", "reverb", "effects"))
    assert torch.equal(files, a[2]) and torch.equal(offs, a[3])
    assert torch.equal(again[0], a[0]) and torch.equal(again[1], a[1])
    files, offs, swapped = by_hand(("pitch", "mix", "effects", "reverb"))
    assert torch.equal(files, a[2]) and torch.equal(offs, a[3]) and not torch.equal(swapped[0], a[0])

    # crops without draws: from the device's default generator, the speed behind the effects
    torch.cuda.manual_seed(13)
    got, got_len = corpus.crops(a[2], a[3], SL, speed=sp, pitch=ps, mix=add, reverb=aug, effects=fx, augment=sa, check=False, **stages, **kw)
    got, got_len = got.clone(), got_len.clone()
    assert (got_len > 0).all() and not torch.equal(got, a[0])

    def by_default_generator(order):
        torch.cuda.manual_seed(13)
        draw = dict(pitch=lambda: ps.draw(6, device=dev), mix=lambda: add.draw(6, SL, sample_rate=rate), reverb=lambda: aug.draw(6, device=dev),
                    effects=lambda: fx.draw(6, rate, device=dev), speed=lambda: sp.draw(6, device=dev))
        drawn = {k: draw[k]() for k in order}
        adraws = sa.draw(lines, got_len.clamp(max=frames))
        return corpus.crops(a[2], a[3], SL, speed=(sp, drawn["speed"]), pitch=(ps, drawn["pitch"]), mix=(add, drawn["mix"]),
                            reverb=(aug, drawn["reverb"]), effects=(fx, drawn["effects"]), augment=(sa, adraws), check=False, **stages, **kw)

    again = by_default_generator(("pitch", "mix", "reverb", "effects", "speed"))
    assert torch.equal(again[0], got) and torch.equal(again[1], got_len)
    assert not torch.equal(by_default_generator(("pitch", "mix", "reverb", "speed", "effects"))[0], got)


def test_a_refused_random_crops_call_leaves_its_generator_where_it_was(staged):
    """What only the stage checks refuse -- a normalize= of a wrong type, a vad.line beyond the line count -- is refused
    before the first draw"""
    import torch

    import alac.net_amd as pkg

    corpus, spec = staged["sig"], pkg.LogMel(SIG_RATE, 400, 160, 80)
    for match, kw in (("normalize must be", dict(normalize="meanvar")),
                      ("vad.line 80 of features with 80 lines", dict(features=spec, vad=pkg.EnergyVad(line=80))),
                      ("features must be", dict(features="logmel", augment=pkg.SpecAugment()))):
        g = torch.Generator(device="cuda").manual_seed(3)
        before = g.get_state().clone()
        with pytest.raises(ValueError, match=match):
            corpus.random_crops(6, SL, generator=g, check=False, **kw)
        assert torch.equal(g.get_state(), before), match
