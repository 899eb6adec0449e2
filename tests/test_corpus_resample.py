"""Corpus.crops(sample_rate=, mono=) on the GPU: a crop at the target rate against the whole file, as `load` returns it,
resampled by the specification (resample.resample_host) and cut -- within the bound of tests/test_resample.py, (N + 2) * 2^-24 *
sum |w x| per element, zeros behind the length; and the defaults against `load` windows bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPEC = [(3, 100, 16), (5, 4000, 24), (1, 9, 16), (4, 4096, 24), (9, 1234, 16)]      # (packets, last packet, bits); 9 frames: less than a filter width


def corpus_files(synth, stereo):
    from test_load_window import make_file

    return [make_file(synth, n, last, ss, stereo, seed=30 + i)[0] for i, (n, last, ss) in enumerate(SPEC)]


def references(pkg, files, rate, mono):
    """Per file (the whole file resampled by the specification, its tolerance): float64 [C or 1, Ty]"""
    from alac.net_amd.resample import resample_host, resample_table

    N = 3 if rate == 44100 else 2 * resample_table(44100, rate)[2] + 1
    refs = []
    for data in files:
        x = pkg.load(data)[0].cpu().numpy().astype(np.float64)
        refs.append((resample_host(x, 44100, rate, mono=mono), (N + 2) * 2.0 ** -24 * resample_host(x, 44100, rate, mono=mono, magnitude=True)))
    return refs


def check_crops(pcm, lengths, refs, cf, co, L, tag):
    got, lens = pcm.cpu().numpy().astype(np.float64), lengths.tolist()
    worst = 0.0
    for b, (f, o) in enumerate(zip(cf, co)):
        want, tol = refs[f]
        n = min(L, want.shape[1] - o)
        assert lens[b] == n, (tag, b, lens[b], n)
        err = np.abs(got[b, :, :n] - want[:, o:o + n])
        if n:
            worst = max(worst, float(np.max(err / np.maximum(tol[:, o:o + n], 1e-300))))
        assert (err <= tol[:, o:o + n]).all(), (tag, b, f, o, float(err.max()))
        assert not got[b, :, n:].any(), (tag, b)
    print(f"{tag}: {len(cf)} crops, worst err / tol {worst:.3f}")


def offsets_of(Ty, L, rng):
    return sorted({0, min(1, Ty), Ty // 2, max(Ty - L, 0), max(Ty - 1, 0), Ty} | {int(rng.integers(0, Ty + 1)) for _ in range(2)})


@pytest.mark.parametrize("stereo", [True, False])
def test_crops_at_a_target_rate_equal_the_resampled_file(synth, stereo):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, stereo)
    rng = np.random.default_rng(6)
    with pkg.Corpus(files) as corpus, pkg.Corpus(files, hbm_bytes=0) as host, \
            pkg.Corpus(files, hbm_bytes=sum(len(f) for f in files[:2])) as split:
        assert host.tier_bytes[0] == 0 and 0 < split.tier_bytes[0] < corpus.tier_bytes[0]
        for rate, mono in ((16000, True), (48000, False), (16000, False), (22050, True), (44100, True)):
            refs = references(pkg, files, rate, mono)
            Ty = corpus.resampled_frames(rate)
            assert Ty.tolist() == [r[0].shape[1] for r in refs]
            for L in (1, 700, 5000):
                crops = [(f, o) for f in range(len(files)) for o in offsets_of(int(Ty[f]), L, rng)]
                cf, co = [c[0] for c in crops], [c[1] for c in crops]
                Co = 1 if mono else corpus.channels
                first = None
                for k, (a, b_) in enumerate(((cf, co), (np.array(cf, dtype=np.int32), np.array(co, dtype=np.uint64)),
                                             (torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")))):
                    out = torch.full((len(crops), Co, L), 12345.0, device="cuda") if k % 2 else None      # out= holding garbage
                    pcm, lengths = corpus.crops(a, b_, L, out=out, sample_rate=rate, mono=mono)
                    assert out is None or pcm is out
                    assert pcm.shape == (len(crops), Co, L) and pcm.dtype == torch.float32 and lengths.dtype == torch.int64 and lengths.device.type == "cuda"
                    if first is None:
                        first = pcm.clone()
                        check_crops(pcm, lengths, refs, cf, co, L, f"{'stereo' if stereo else 'mono'} file -> {rate} mono={mono} L={L}")
                    assert torch.equal(pcm, first), (rate, L, k)
                # the tiers underneath change nothing
                for other in (host, split):
                    pcm, lengths2 = other.crops(cf, co, L, sample_rate=rate, mono=mono)
                    assert torch.equal(pcm, first) and torch.equal(lengths2, lengths), (rate, L)
        # the host-side checks, at the target rate, before any device work
        Ty = corpus.resampled_frames(16000)
        for a, b_, L in (([0, 1], [0], 10), ([5], [0], 10), ([-1], [0], 10), ([0], [int(Ty[0]) + 1], 10), ([0], [-1], 10), ([0], [0], -1)):
            with pytest.raises(ValueError):
                corpus.crops(a, b_, L, sample_rate=16000)
        corpus.crops([0], [int(Ty[0])], 10, sample_rate=16000)
        with pytest.raises(ValueError, match="float32"):
            corpus.crops([0], [0], 10, dtype=torch.int32, sample_rate=16000)
        with pytest.raises(ValueError, match="out must be"):
            corpus.crops([0], [0], 10, sample_rate=16000, mono=True, out=torch.zeros((1, corpus.channels + 1, 10), device="cuda"))
        with pytest.raises(ValueError, match="16384"):
            corpus.crops([0], [0], 10, sample_rate=44099)
        # device indices outside the corpus: a length code, a row of zeros, and a ValueError naming the crop when checked
        a, b_ = torch.tensor([0, 7, 1, 0], device="cuda"), torch.tensor([3, 0, 10 ** 9, -1], device="cuda")
        pcm, lengths = corpus.crops(a, b_, 50, sample_rate=16000, check=False)
        assert lengths.tolist() == [50, -1, -1, -1] and not pcm[1:].any() and pcm[0].any()
        with pytest.raises(ValueError, match="crop 1"):
            corpus.crops(a, b_, 50, sample_rate=16000)
        # nothing to do
        pcm, lengths = corpus.crops([], [], 100, sample_rate=16000)
        assert pcm.shape == (0, corpus.channels, 100) and lengths.shape == (0,)
        pcm, lengths = corpus.crops([0, 1], [5, 0], 0, sample_rate=16000, mono=True)
        assert pcm.shape == (2, 1, 0) and lengths.tolist() == [0, 0]


def test_the_defaults_and_the_corpus_rate_are_the_load_windows(synth):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, True)
    with pkg.Corpus(files) as corpus:
        cf, co, L = [0, 1, 2, 3, 4, 4], [50, 4000, 0, 8191, 30000, int(corpus.num_frames[4])], 3000
        for dtype in (torch.float32, torch.int32):
            want = torch.zeros((len(cf), 2, L), dtype=dtype, device="cuda")
            for b, (f, o) in enumerate(zip(cf, co)):
                one, _ = pkg.load(files[f], dtype=dtype, frame_offset=o, num_frames=L)
                want[b, :, :one.shape[1]] = one
            for kw in (dict(), dict(sample_rate=None, mono=False), dict(sample_rate=44100)):
                pcm, lengths = corpus.crops(cf, co, L, dtype=dtype, **kw)
                assert torch.equal(pcm, want) and pcm.dtype == dtype, kw
        # mono alone: the mean of the two channels in float32, exactly
        pcm, lengths = corpus.crops(cf, co, L, mono=True)
        full, _ = corpus.crops(cf, co, L)
        assert pcm.shape == (len(cf), 1, L) and torch.equal(pcm[:, 0], (full[:, 0] + full[:, 1]) * 0.5)
        assert lengths.tolist() == [min(L, int(corpus.num_frames[f]) - o) for f, o in zip(cf, co)]


def test_unchecked_resampled_crops_read_nothing_back_and_reuse_their_arrays(synth):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, True)
    with pkg.Corpus(files) as corpus:
        cf, co = torch.tensor([0, 1, 4, 3], device="cuda"), torch.tensor([5, 1500, 11000, 0], device="cuda")
        want, want_len = corpus.crops(cf, co, 2000, sample_rate=16000, mono=True)     # (also the first call's allocations)
        g = torch.Generator(device="cuda")
        corpus.random_crops(16, 2000, generator=g, sample_rate=16000, mono=True)
        out = torch.empty_like(want)
        scratch = corpus._rs_scratch.data_ptr()
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                want_len.cpu()
            pcm, lengths = corpus.crops(cf, co, 2000, sample_rate=16000, mono=True, check=False)
            pcm2, lengths2 = corpus.crops(cf, co, 2000, sample_rate=16000, mono=True, check=False, out=out)
            r = corpus.random_crops(16, 2000, generator=g, sample_rate=16000, mono=True, check=False)
            with pytest.raises(RuntimeError):
                corpus.crops(cf, co, 2000, sample_rate=16000, mono=True, check=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(pcm, want) and torch.equal(pcm2, want) and torch.equal(lengths, want_len) and pcm2 is out
        assert r[0].shape == (16, 1, 2000) and corpus._rs_scratch.data_ptr() == scratch
        del pcm, lengths, pcm2, lengths2, r
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == allocated      # no step allocated anything it kept


def test_random_resampled_crops_are_inside_their_files_and_reproducible(synth):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, True)
    with pkg.Corpus(files) as corpus:
        Ty = torch.from_numpy(corpus.resampled_frames(16000))
        assert Ty.tolist() == [-(-160 * int(n) // 441) for n in corpus.num_frames]
        for L in (100, 3000):
            g = torch.Generator(device="cuda")
            g.manual_seed(7)
            pcm, lengths, cf, co = corpus.random_crops(300, L, generator=g, sample_rate=16000, mono=True)
            f, o = cf.cpu(), co.cpu()
            assert pcm.shape == (300, 1, L) and ((f >= 0) & (f < 5)).all() and (o >= 0).all() and (o <= (Ty[f] - L).clamp(min=0)).all()
            assert len(set(f.tolist())) == 5 and len(set(o.tolist())) > 100
            assert torch.equal(lengths.cpu(), torch.minimum(Ty[f] - o, torch.tensor(L)))
            again, lengths2 = corpus.crops(cf, co, L, sample_rate=16000, mono=True)
            assert torch.equal(pcm, again) and torch.equal(lengths, lengths2)
            g.manual_seed(7)
            pcm2, _, cf2, co2 = corpus.random_crops(300, L, generator=g, sample_rate=16000, mono=True)
            assert torch.equal(cf, cf2) and torch.equal(co, co2) and torch.equal(pcm, pcm2)


def test_a_corrupt_packet_is_named_in_a_resampled_crop(synth):
    import torch

    import alac.net_amd as pkg
    from test_load_window import corrupt, make_file

    data, _ = make_file(synth, 6, 2000)
    with pkg.Corpus([corrupt(data, 2)]) as corpus:              # frames 8192 .. 12288 do not decode: 2972 .. 4459 at 16 kHz
        with pytest.raises(pkg.AlacGpuError, match=r"crop 1 \(source 0\), packet 2 does not decode"):
            corpus.crops([0, 0], [0, 3000], 500, sample_rate=16000)
        pcm, lengths = corpus.crops([0, 0], [0, 3200], 500, sample_rate=16000, check=False)
        assert lengths.tolist() == [500, 500] and pcm[0].any() and not pcm[1].any()      # the packet's run is zeros
