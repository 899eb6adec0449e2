"""Corpus(sources, mixed_rates=True) on the GPU: crops at one target rate of files of four sample rates against every file, as
`load` returns it, resampled by the specification with the file's own rates (resample.resample_host) and cut -- within the
bound of tests/test_corpus_resample.py, (N_f + 2) * 2^-24 * sum |w x| per element with file f's own N_f (3 for the file that
is at the target rate already: the table that copies), zeros behind the length; and bit for bit against the single-file
corpora, whose crops go through the one-table kernel: mixing changes nothing."""
import io

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
def mixed(tmp_path_factory):
    """The four files (written by `save`), and per file and mono: (the whole file resampled by the specification, its tolerance)"""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_host, resample_table

    d = tmp_path_factory.mktemp("mixed_rates")
    paths, refs = [], {False: [], True: []}
    for i, (rate, frames, bits, fl) in enumerate(SPEC):
        path = str(d / f"f{i}_{rate}.m4a")
        pkg.save(path, signal(torch, rate, frames, 50 + i), rate, sample_size=bits, frame_length=fl)
        paths.append(path)
        x = pkg.load(path)[0].cpu().numpy().astype(np.float64)
        assert x.shape == (2, frames)
        N = 3 if rate == TARGET else 2 * resample_table(rate, TARGET)[2] + 1
        for mono in (False, True):
            refs[mono].append((resample_host(x, rate, TARGET, mono=mono), (N + 2) * 2.0 ** -24 * resample_host(x, rate, TARGET, mono=mono, magnitude=True)))
    return paths, refs


def the_crops(Ty):
    """24 crops: per file its first frames, its last frames running past the end, and four middles"""
    rng = np.random.default_rng(9)
    crops = []
    for f, n in enumerate(Ty):
        n = int(n)
        crops += [(f, 0), (f, n - 700), (f, n // 2)] + [(f, int(o)) for o in rng.integers(1, n - L, 3)]
    return [c[0] for c in crops], [c[1] for c in crops]


def check_crops(pcm, lengths, refs, cf, co, tag):
    got, lens = pcm.cpu().numpy().astype(np.float64), lengths.tolist()
    worst = 0.0
    for b, (f, o) in enumerate(zip(cf, co)):
        want, tol = refs[f]
        n = min(L, want.shape[1] - o)
        assert lens[b] == n, (tag, b, lens[b], n)
        err = np.abs(got[b, :, :n] - want[:, o:o + n])
        worst = max(worst, float(np.max(err / np.maximum(tol[:, o:o + n], 1e-300))))
        assert (err <= tol[:, o:o + n]).all(), (tag, b, f, o, float(err.max()))
        assert not got[b, :, n:].any(), (tag, b)
        assert got[b, :, :n].any(), (tag, b)
    print(f"{tag}: {len(cf)} crops, worst err / tol {worst:.3f}")


@pytest.mark.parametrize("mono", [False, True])
def test_crops_of_files_of_four_rates_equal_the_resampled_files(mixed, mono):
    import torch

    import alac.net_amd as pkg

    paths, refs = mixed
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        assert corpus.sample_rate is None and corpus.sample_rates.tolist() == [s[0] for s in SPEC] and corpus.sample_rates.dtype == np.int64
        assert corpus.num_frames.tolist() == [s[1] for s in SPEC]              # source frames
        Ty = corpus.resampled_frames(TARGET)
        ratios = [(441, 160), (3, 1), (1, 1), (441, 320)]
        assert Ty.tolist() == [-(-b * s[1] // a) for (a, b), s in zip(ratios, SPEC)] == [r[0].shape[1] for r in refs[mono]]
        cf, co = the_crops(Ty)
        assert len(cf) == 24
        pcm, lengths = corpus.crops(cf, co, L, sample_rate=TARGET, mono=mono)
        assert pcm.shape == (24, 1 if mono else 2, L) and pcm.dtype == torch.float32 and lengths.dtype == torch.int64
        check_crops(pcm, lengths, refs[mono], cf, co, f"mono={mono}")
        assert lengths.tolist()[1] == 700
        # device indices and out= holding garbage: the same crops
        out = torch.full_like(pcm, 12345.0)
        pcm2, lengths2 = corpus.crops(torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda"), L, sample_rate=TARGET, mono=mono, out=out)
        assert pcm2 is out and torch.equal(pcm2, pcm) and torch.equal(lengths2, lengths)
        # mixing changes nothing: the four single-file corpora give these crops bit for bit
        for f, path in enumerate(paths):
            rows = [b for b in range(24) if cf[b] == f]
            with pkg.Corpus([path]) as single:
                assert single.sample_rate == SPEC[f][0]
                one, one_len = single.crops([0] * len(rows), [co[b] for b in rows], L, sample_rate=TARGET, mono=mono)
                assert torch.equal(pcm[rows], one) and torch.equal(lengths[rows], one_len), f
                if SPEC[f][0] == TARGET and not mono:      # the file at the target rate: the plain decode
                    plain, plain_len = single.crops([0] * len(rows), [co[b] for b in rows], L)
                    assert torch.equal(pcm[rows], plain) and torch.equal(lengths[rows], plain_len)
        # host checks at the target rate, before any device work
        for a, b_ in (([0, 1], [0]), ([4], [0]), ([0], [int(Ty[0]) + 1]), ([2], [-1])):
            with pytest.raises(ValueError):
                corpus.crops(a, b_, L, sample_rate=TARGET, mono=mono)
        pcm0, len0 = corpus.crops([1], [int(Ty[1])], 10, sample_rate=TARGET, mono=mono)
        assert len0.tolist() == [0] and not pcm0.any()


def test_a_rate_is_required_and_a_table_that_is_too_large_names_its_file(mixed):
    import torch

    import alac.net_amd as pkg

    paths, _ = mixed
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        with pytest.raises(ValueError, match="sample_rate"):
            corpus.crops([0], [0], L)
        with pytest.raises(ValueError, match="sample_rate"):
            corpus.crops([0], [0], L, mono=True)
        with pytest.raises(ValueError, match="sample_rate"):
            corpus.random_crops(4, L)
        with pytest.raises(ValueError, match=r"source 0: .*16384"):
            corpus.crops([2], [0], L, sample_rate=44099)
        with pytest.raises(ValueError, match=r"source 1: .*16384"):      # 44100 Hz to 1764 Hz is 25 : 1, 48000 Hz to 1764 Hz is 4000 : 147
            corpus.crops([0], [0], L, sample_rate=1764)
        with pytest.raises(ValueError, match="float32"):
            corpus.crops([0], [0], L, sample_rate=TARGET, dtype=torch.int32)
        with pytest.raises(ValueError):
            corpus.crops([0], [0], L, sample_rate=0)
        pcm, lengths = corpus.crops([], [], L, sample_rate=TARGET)
        assert pcm.shape == (0, 2, L) and lengths.shape == (0,)
    # the default still refuses such files
    with pytest.raises(ValueError, match="source 1: 2 channels at 48000 Hz, the first has 2 at 44100 Hz"):
        pkg.Corpus(paths)


def test_device_indices_outside_the_corpus_and_unchecked_calls_read_nothing_back(mixed):
    import torch

    import alac.net_amd as pkg

    paths, _ = mixed
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        cf, co = torch.tensor([0, 7, 1, 2, 3], device="cuda"), torch.tensor([3, 0, 10 ** 9, -1, 40], device="cuda")
        pcm, lengths = corpus.crops(cf, co, 50, sample_rate=TARGET, check=False)
        assert lengths.tolist() == [50, -1, -1, -1, 50] and not pcm[1:4].any() and pcm[0].any() and pcm[4].any()
        with pytest.raises(ValueError, match="crop 1"):
            corpus.crops(cf, co, 50, sample_rate=TARGET)
        del pcm, lengths
        cf, co = torch.tensor([0, 1, 3, 2], device="cuda"), torch.tensor([5, 1500, 9000, 0], device="cuda")
        want, want_len = corpus.crops(cf, co, L, sample_rate=TARGET, mono=True)     # (also the first call's allocations)
        g = torch.Generator(device="cuda")
        corpus.random_crops(16, L, generator=g, sample_rate=TARGET, mono=True)
        out = torch.empty_like(want)
        scratch = corpus._rs_scratch.data_ptr()
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                want_len.cpu()
            pcm, lengths = corpus.crops(cf, co, L, sample_rate=TARGET, mono=True, check=False)
            pcm2, lengths2 = corpus.crops(cf, co, L, sample_rate=TARGET, mono=True, check=False, out=out)
            r = corpus.random_crops(16, L, generator=g, sample_rate=TARGET, mono=True, check=False)
            with pytest.raises(RuntimeError):
                corpus.crops(cf, co, L, sample_rate=TARGET, mono=True, check=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(pcm, want) and torch.equal(pcm2, want) and torch.equal(lengths, want_len) and pcm2 is out
        assert r[0].shape == (16, 1, L) and corpus._rs_scratch.data_ptr() == scratch
        del pcm, lengths, pcm2, lengths2, r
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == allocated      # no step allocated anything it kept


def test_a_crop_plans_the_packets_of_its_own_source_window(mixed):
    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_table, source_window

    paths, _ = mixed
    with pkg.Corpus(paths, mixed_rates=True) as corpus, pkg.Corpus(paths[2:3]) as only16, pkg.Corpus(paths[1:2]) as only48:
        # full windows: first frames and middles of the 16 kHz file (rows 0 .. 2) and of the 48 kHz file (rows 3 .. 5)
        cf, co = [2, 2, 2, 1, 1, 1], [0, 3000, 7777, 0, 2000, 4001]
        corpus.crops(cf, co, L, sample_rate=TARGET, check=False)
        status, is_packet = corpus.last_status()
        K = corpus.entries_per_crop(L, sample_rate=TARGET)
        assert is_packet.shape == (len(cf) * K,) and status.shape == is_packet.shape
        used = is_packet.view(len(cf), K).sum(dim=1).tolist()
        Ls16 = source_window(0, L, 1, 1, 1)[1]
        Ls48 = source_window(0, L, *resample_table(48000, TARGET)[:3])[1]
        assert (Ls16, Ls48) == (1503, 4541)
        K16, K48 = only16.entries_per_crop(Ls16), only48.entries_per_crop(Ls48)
        assert K == K48 == 6 and K16 == 3        # 4541 and 1503 frames of 1024-frame packets
        assert all(u <= K16 for u in used[:3]) and all(u > K16 for u in used[3:]), used
        assert (status[is_packet] == 0).all()
        # the bound of a file is that of its own window, not of the longest
        assert K16 < only16.entries_per_crop(Ls48)


def test_a_host_tier_underneath_changes_nothing(mixed):
    import os

    import torch

    import alac.net_amd as pkg

    paths, _ = mixed
    sizes = [os.path.getsize(p) for p in paths]
    with pkg.Corpus(paths, mixed_rates=True) as corpus, pkg.Corpus(paths, mixed_rates=True, hbm_bytes=sizes[0] + sizes[1]) as split:
        assert split.tier_bytes[0] > 0 and split.tier_bytes[1] > 0 and corpus.tier_bytes[1] == 0
        packets = np.diff(split._host["file_base"].astype(np.int64))
        assert split.tier_bytes == (int(packets[:2].sum()), int(packets[2:].sum()))      # two files on the host tier
        cf, co = the_crops(corpus.resampled_frames(TARGET))
        for mono in (False, True):
            want, want_len = corpus.crops(cf, co, L, sample_rate=TARGET, mono=mono)
            got, got_len = split.crops(cf, co, L, sample_rate=TARGET, mono=mono)
            assert torch.equal(got, want) and torch.equal(got_len, want_len)
            S = split.stage_bytes_per_crop(L, sample_rate=TARGET)
            staged = int(split.last_staged_bytes())
            assert 0 < staged <= len(cf) * S
        assert corpus.last_staged_bytes() is None


def test_random_crops_are_inside_their_files_and_reproducible(mixed):
    import torch

    import alac.net_amd as pkg

    paths, _ = mixed
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        Ty = torch.from_numpy(corpus.resampled_frames(TARGET))
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        pcm, lengths, cf, co = corpus.random_crops(64, L, generator=g, sample_rate=TARGET)
        f, o = cf.cpu(), co.cpu()
        assert pcm.shape == (64, 2, L) and ((f >= 0) & (f < 4)).all() and (o >= 0).all() and (o <= (Ty[f] - L).clamp(min=0)).all()
        assert len(set(f.tolist())) == 4 and len(set(o.tolist())) > 32
        assert (lengths == L).all()
        again, lengths2 = corpus.crops(cf, co, L, sample_rate=TARGET)
        assert torch.equal(pcm, again) and torch.equal(lengths, lengths2)
        g.manual_seed(7)
        pcm2, _, cf2, co2 = corpus.random_crops(64, L, generator=g, sample_rate=TARGET)
        assert torch.equal(cf, cf2) and torch.equal(co, co2) and torch.equal(pcm, pcm2)


def test_files_of_one_rate_make_the_corpus_of_the_default(mixed):
    import torch

    import alac.net_amd as pkg

    files = []
    for i, (frames, bits, fl) in enumerate(((9000, 16, 4096), (5000, 24, 1024), (700, 16, 4096))):
        buf = io.BytesIO()
        pkg.save(buf, signal(torch, 44100, frames, 70 + i), 44100, sample_size=bits, frame_length=fl)
        files.append(buf.getvalue())
    with pkg.Corpus(files) as plain, pkg.Corpus(files, mixed_rates=True) as same:
        assert same.sample_rate == plain.sample_rate == 44100 and same.sample_rates.tolist() == plain.sample_rates.tolist() == [44100] * 3
        cf, co = [0, 1, 2, 0, 1], [0, 1500, 100, 3000, 17]
        for kw in (dict(), dict(dtype=torch.int32), dict(sample_rate=None), dict(sample_rate=44100), dict(mono=True), dict(sample_rate=TARGET),
                   dict(sample_rate=TARGET, mono=True), dict(sample_rate=48000)):
            a, a_len = plain.crops(cf, co, 1000, **kw)
            b, b_len = same.crops(cf, co, 1000, **kw)
            assert a.dtype == b.dtype and torch.equal(a, b) and torch.equal(a_len, b_len), kw
        assert same.resampled_frames(TARGET).tolist() == plain.resampled_frames(TARGET).tolist()
        assert same.entries_per_crop(1000) == plain.entries_per_crop(1000)
        ga, gb = torch.Generator(device="cuda"), torch.Generator(device="cuda")
        ga.manual_seed(3)
        gb.manual_seed(3)
        for kw in (dict(), dict(sample_rate=TARGET, mono=True)):
            ra, rb = plain.random_crops(8, 500, generator=ga, **kw), same.random_crops(8, 500, generator=gb, **kw)
            assert all(torch.equal(x, y) for x, y in zip(ra, rb)), kw


def test_a_saved_corpus_is_the_same_corpus(mixed, tmp_path):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import container

    paths, _ = mixed
    saved = [str(tmp_path / f"saved{f}.m4a") for f in range(4)]
    with pkg.Corpus(paths, mixed_rates=True) as corpus:
        corpus.save(saved)                      # every file at its own rate
        cf, co = the_crops(corpus.resampled_frames(TARGET))
        want, want_len = corpus.crops(cf, co, L, sample_rate=TARGET)
        with pytest.raises(ValueError):
            corpus.save(saved, sample_rate=0)
    assert [int(container.packet_table(p)["sample_rate"]) for p in saved] == [s[0] for s in SPEC]
    with pkg.Corpus(saved, mixed_rates=True) as again:
        assert again.sample_rates.tolist() == [s[0] for s in SPEC] and again.sample_rate is None
        got, got_len = again.crops(cf, co, L, sample_rate=TARGET)
        assert torch.equal(got, want) and torch.equal(got_len, want_len)


def test_a_corrupt_packet_is_named_in_a_crop(mixed):
    import alac.net_amd as pkg
    from test_load_window import corrupt

    paths, _ = mixed
    good = [open(p, "rb").read() for p in paths]
    # packet 2 of the 48 kHz file (1024-frame packets) does not decode: its frames 2048 .. 3072 are 683 .. 1024 at 16 kHz
    with pkg.Corpus([good[0], corrupt(good[1], 2), good[2], good[3]], mixed_rates=True) as corpus:
        with pytest.raises(pkg.AlacGpuError, match=r"crop 2 \(source 1\), packet 2 does not decode"):
            corpus.crops([0, 1, 1], [0, 3000, 500], 400, sample_rate=TARGET)
        pcm, lengths = corpus.crops([0, 1, 1], [0, 3000, 720], 250, sample_rate=TARGET, check=False)
        assert lengths.tolist() == [250, 250, 250] and pcm[0].any() and pcm[1].any() and not pcm[2].any()      # the packet's run is zeros
