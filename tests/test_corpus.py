"""alac.Corpus on the GPU: the crop planner (alacgpu_plan_crops_device) against its host twin, and crops of a resident corpus
bit-equal to `load` of the same window -- exact: nothing on this path has a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 16


def make_file(synth, n_packets, last, sample_size=16, stereo=True, seed=5):
    from test_load_window import make_file as make

    return make(synth, n_packets, last, sample_size, stereo, seed)


def plan_tables(rng):
    """Duration tables of every kind the planner meets, as resident tables (numpy): regular files, a one-packet file,
    zero-duration packets, a duration above 16384, files without frames or packets, and a file of 9000 irregular packets (the
    searches' second level)."""
    from test_corpus_plan import TABLES, tables_of

    files = [list(t) for t in TABLES] + [[4096] * 700 + [33], rng.choice([0, 1, 17, 1000, 4096, 16384], 9000).tolist(), [4096] * 64]
    return files, tables_of(files, rng)


def edge_crops(files):
    from test_corpus_plan import edge_offsets

    return [(f, o) for f, d in enumerate(files) if len(d) < 100 for o in edge_offsets(d)]


def run_planner(torch, pkg, ctx, tb, crop_file, crop_offset, L, K, stride):
    """alacgpu_plan_crops_device into arrays with GUARD elements of 0x5A bytes in front of and behind them; returns the seven
    arrays (device tensors, the unsigned types as their signed twins) and whether every guard is intact"""
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if len(a) else np.zeros(1, dt)).to(dev)
    d_tab = [up(tb["pkt_offset"], np.int64), up(tb["pkt_size"], np.int32), up(tb["pkt_end"], np.int64), up(tb["file_first"], np.int32),
             up(tb["file_cfg"], np.int16)]
    B = len(crop_file)
    d_cf = up(np.asarray(crop_file, dtype=np.uint32), np.int32)
    d_co = up(np.asarray(crop_offset, dtype=np.uint64), np.int64)
    kinds = [torch.int64, torch.int32, torch.int16, torch.int64, torch.int32, torch.int32, torch.int64]
    counts = [B * K] * 6 + [B]
    raw = [torch.full(((n + 2 * GUARD) * torch.empty(0, dtype=k).element_size(),), 0x5A, dtype=torch.uint8, device=dev).view(k)
           for n, k in zip(counts, kinds)]
    outs = [r[GUARD:GUARD + n] for r, n in zip(raw, counts)]
    rc = pkg.lib().alacgpu_plan_crops_device(ctx._ctx, *[pkg._dp(t) for t in d_tab], len(tb["file_first"]) - 1, pkg._dp(d_cf),
                                             pkg._dp(d_co), B, L, K, stride, *[pkg._dp(t) for t in outs],
                                             pkg._VP(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    intact = all(bool((torch.cat([r[:GUARD], r[GUARD + n:]]).view(torch.uint8) == 0x5A).all()) for r, n in zip(raw, counts))
    return outs, intact


def test_planner_equals_its_host_twin():
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(17)
    files, tb = plan_tables(rng)
    F = len(files)
    totals = [int(np.sum(d)) for d in files]
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.int64): np.int64}
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        # (L, K or None for the corpus's own K(L), B): B not a multiple of 64 nor of the four crops of a workgroup; K 1; K above
        # 64 both as the bound of a long window and as mostly padding; a K that is too small for many crops
        for L, K, B in ((4096, None, 301), (1, 1, 130), (88200, None, 257), (70 * 4096, None, 66), (17, 100, 67), (3 * 4096, 2, 203),
                        (0, 3, 9), (2 ** 32 - 1, 5, 31)):
            if K is None:
                K = max(pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L), 1)
            # outside the corpus: a file that does not exist, an offset past the end, the largest values
            crops = [(F, 0), (F + 7, 5), (2 ** 32 - 1, 0), (0, totals[0] + 1), (8, 2 ** 64 - 1), (9, 2 ** 63)]
            crops += [(8, 4095), (8, 3 * 4096 + 1)]     # (in the file of 700 packets of 4096: a long window's K entries, all used)
            crops += edge_crops(files) if L in (4096, 17, 3 * 4096) else []
            while len(crops) < B or len(crops) % 4 == 0:
                f = int(rng.integers(0, F))
                crops.append((f, int(rng.integers(0, totals[f] + 1))))
            cf = np.array([c[0] for c in crops], dtype=np.uint32)
            co = np.array([c[1] for c in crops], dtype=np.uint64)
            stride = 2 * L
            want = pkg.corpus_plan_host(tb["pkt_offset"], tb["pkt_size"], tb["pkt_end"], tb["file_first"], tb["file_cfg"], cf, co,
                                        L, K, stride)
            got, intact = run_planner(torch, pkg, ctx, tb, cf, co, L, K, stride)
            assert intact, f"a store outside the plan arrays (L {L}, K {K})"
            names = ("offsets", "sizes", "cfg_idx", "dst_first", "dst_frames", "src_skip", "lengths")
            for name, g, w in zip(names, got, want):
                w = torch.from_numpy(w.view(signed[w.dtype]))
                assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (name, L, K, torch.nonzero(g.cpu() != w)[:5].tolist())
            assert (want[6][:6] == -1).all() and (want[6][6:] != -1).all()
            if (L, K) == (3 * 4096, 2):
                assert (want[6] == -2).sum() > 20
            if L == 70 * 4096:
                assert K > 64 and (want[2].reshape(-1, K)[6, :71] != 0xFFFF).all()      # entries past a lane's first are used
        # the argument checks: a no-op, K 0, too many entries, a NULL and a misaligned array
        L_ = pkg.lib()
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        p, q = pkg._dp(t), pkg._VP(t.data_ptr() + 1)
        args = lambda **kw: [ctx._ctx, p, p, p, p, p, 1, p, p, kw.get("B", 1), 1, kw.get("K", 1), 0,
                             kw.get("first", p), p, p, p, p, p, p, None]
        assert L_.alacgpu_plan_crops_device(*args(B=0, K=0)) == 0
        assert L_.alacgpu_plan_crops_device(*args(K=0)) == -1
        assert L_.alacgpu_plan_crops_device(*args(B=65536, K=65536)) == -1
        assert L_.alacgpu_plan_crops_device(*args(first=None)) == -1
        assert L_.alacgpu_plan_crops_device(*args(first=q)) == -1
        torch.cuda.synchronize()


def corpus_files(synth, stereo):
    """(file bytes, source PCM [T, C], sample size) of a small corpus: 16- and 24-bit, mixed packet counts, short last packets,
    a one-packet file"""
    spec = [(3, 100, 16), (5, 4000, 24), (1, 17, 16), (4, 4096, 24), (9, 1234, 16)]
    return [make_file(synth, n, last, ss, stereo, seed=10 + i) + (ss,) for i, (n, last, ss) in enumerate(spec)]


def some_crops(files, L, rng):
    from test_corpus_plan import edge_offsets

    crops = []
    for f, (_, pcm, _) in enumerate(files):
        T = len(pcm)
        offs = sorted({0, 1, T - 1, T, min(4095, T), min(4096, T), min(4097, T), max(T - L, 0)} | {int(rng.integers(0, T + 1)) for _ in range(2)})
        crops += [(f, o) for o in offs]
    return crops


@pytest.mark.parametrize("stereo", [True, False])
def test_crops_equal_load_of_the_same_window(synth, stereo):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, stereo)
    rng = np.random.default_rng(4)
    with pkg.Corpus([f[0] for f in files]) as corpus:
        assert corpus.num_files == 5 and corpus.channels == (2 if stereo else 1) and corpus.sample_rate == 44100
        assert corpus.num_frames.tolist() == [len(f[1]) for f in files] and corpus.num_frames.dtype == np.int64
        assert len(corpus._gpu.cfgs) == 2           # five files, two stream cfgs
        for L in (1, 3000, 2 * 4096 + 1):
            crops = some_crops(files, L, rng)
            cf, co = [c[0] for c in crops], [c[1] for c in crops]
            for dtype in (torch.float32, torch.int32):
                want = torch.zeros((len(crops), corpus.channels, L), dtype=dtype)
                want_len = []
                for b, (f, o) in enumerate(crops):
                    one, _ = pkg.load(files[f][0], dtype=dtype, frame_offset=o, num_frames=L)
                    want[b, :, :one.shape[1]] = one.cpu()
                    want_len.append(one.shape[1])
                # host indices (lists, numpy), device indices, and out= holding garbage
                for k, (a, b_) in enumerate(((cf, co), (np.array(cf, dtype=np.int32), np.array(co, dtype=np.uint64)),
                                             (torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")),
                                             (torch.tensor(cf, device="cuda", dtype=torch.int32), torch.tensor(co, device="cuda")))):
                    out = None
                    if k % 2:
                        out = torch.full((len(crops), corpus.channels, L), 12345, dtype=dtype, device="cuda")
                    pcm, lengths = corpus.crops(a, b_, L, dtype=dtype, out=out)
                    assert out is None or pcm is out
                    assert pcm.dtype == dtype and pcm.shape == want.shape and lengths.device.type == "cuda" and lengths.dtype == torch.int64
                    assert lengths.tolist() == want_len, (L, k)
                    assert torch.equal(pcm.cpu(), want), (L, dtype, k)
        # nothing to decode: empty tensors, no launch
        pcm, lengths = corpus.crops([], [], 100)
        assert pcm.shape == (0, corpus.channels, 100) and lengths.shape == (0,)
        pcm, lengths = corpus.crops([0, 1], [5, 0], 0, dtype=torch.int32)
        assert pcm.shape == (2, corpus.channels, 0) and lengths.tolist() == [0, 0]
        # the host-side checks come before any device work
        for a, b_, L in (([0, 1], [0], 10), ([5], [0], 10), ([-1], [0], 10), ([0], [len(files[0][1]) + 1], 10), ([0], [-1], 10),
                         ([0], [0], -1), ([0.5], [0], 10)):
            with pytest.raises(ValueError):
                corpus.crops(a, b_, L)
        with pytest.raises(ValueError):
            corpus.crops([0], [0], 10, out=torch.zeros((1, corpus.channels, 11), device="cuda"))
        # device indices outside the corpus: a length code, a row of zeros, and a ValueError when checked
        a, b_ = torch.tensor([0, 7, 1], device="cuda"), torch.tensor([3, 0, 10 ** 9], device="cuda")
        pcm, lengths = corpus.crops(a, b_, 50, dtype=torch.int32, check=False)
        assert lengths.tolist() == [50, -1, -1] and not pcm[1:].any() and pcm[0].any()
        with pytest.raises(ValueError, match="crop 1"):
            corpus.crops(a, b_, 50)


def test_crops_that_share_packets_are_each_right(synth):
    import torch

    import alac.net_amd as pkg

    data, pcm = make_file(synth, 6, 2000)
    other, pcm2 = make_file(synth, 2, 50, seed=2)
    with pkg.Corpus([data, other, data]) as corpus:
        cf = [0, 0, 0, 2, 1, 0, 2]
        co = [4000, 4000, 4100, 4000, 0, 0, 8191]
        out, lengths = corpus.crops(cf, co, 5000, dtype=torch.int32)
        assert lengths.tolist() == [5000, 5000, 5000, 5000, 4096 + 50, 5000, 5000]
        o = out.cpu()
        for b, (f, off) in enumerate(zip(cf, co)):
            src = pcm2 if f == 1 else pcm
            n = int(lengths[b])
            assert torch.equal(o[b, :, :n], torch.from_numpy(src[off:off + n].astype(np.int32)).T), b
            assert not o[b, :, n:].any()


def test_a_corrupt_packet_is_named_or_left_as_zeros(synth):
    import torch

    import alac.net_amd as pkg
    from test_load_window import corrupt

    data, pcm = make_file(synth, 6, 2000)
    good, pcm_good = make_file(synth, 4, 4096, seed=9)
    bad = corrupt(data, 2)                     # frames 8192 .. 12288 of source 1 do not decode
    with pkg.Corpus([good, bad]) as corpus:
        out, lengths = corpus.crops([0, 1, 1, 1], [100, 0, 12288, 100], 8000, dtype=torch.int32)
        want = [pcm_good[100:8100], pcm[0:8000], pcm[12288:20288], pcm[100:8100]]
        for b, w in enumerate(want):
            assert torch.equal(out[b].cpu(), torch.from_numpy(w.astype(np.int32)).T.contiguous()), b
        for cf, co, L, crop in (([0, 1], [0, 8191], 2, 1), ([1, 0, 1], [12287, 5, 0], 10, 0), ([0, 0, 1], [0, 1, 4000], 8000, 2)):
            with pytest.raises(pkg.AlacGpuError, match=f"crop {crop} \\(source 1\\), packet 2 does not decode: status [36] "):
                corpus.crops(cf, co, L)
            with pytest.raises(pkg.AlacGpuError, match=f"crop {crop} \\(source 1\\), packet 2 "):
                corpus.crops(torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda"), L)
        # unchecked: nothing raises, the packet's run is zeros, the rest of the row is right, and the status sits at its entry
        out, lengths = corpus.crops([0, 1], [0, 4000], 10000, dtype=torch.int32, check=False)
        o = out.cpu()
        assert torch.equal(o[0], torch.from_numpy(pcm_good[0:10000].astype(np.int32)).T.contiguous())
        row = pcm[4000:14000].astype(np.int32).copy()
        row[8192 - 4000:12288 - 4000] = 0
        assert torch.equal(o[1], torch.from_numpy(row).T.contiguous())
        st, valid = corpus.last_status()
        K = corpus.entries_per_crop(10000)
        assert K == 4 and st.shape == (2 * K,) and valid.shape == (2 * K,) and st.device.type == "cuda"
        assert valid.tolist() == [True, True, True, False, True, True, True, True]
        s = st.tolist()
        assert s[:3] == [0, 0, 0] and s[4:6] == [0, 0] and s[6] in (3, 6) and s[7] == 0


def test_random_crops_are_inside_their_files_and_reproducible(synth):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, True)
    with pkg.Corpus([f[0] for f in files]) as corpus:
        T = torch.from_numpy(corpus.num_frames)
        for L in (100, 5000, 40000):
            g = torch.Generator(device="cuda")
            g.manual_seed(7)
            pcm, lengths, cf, co = corpus.random_crops(300, L, generator=g, dtype=torch.int32)
            assert cf.device.type == "cuda" and co.device.type == "cuda" and pcm.shape == (300, 2, L)
            f, o = cf.cpu(), co.cpu()
            assert ((f >= 0) & (f < 5)).all() and (o >= 0).all() and (o <= (T[f] - L).clamp(min=0)).all()
            assert len(set(f.tolist())) == 5 and (L > 5000 or len(set(o.tolist())) > 100)
            assert torch.equal(lengths.cpu(), torch.minimum(T[f] - o, torch.tensor(L)))
            again, lengths2 = corpus.crops(cf, co, L, dtype=torch.int32)
            assert torch.equal(pcm, again) and torch.equal(lengths, lengths2)
            g.manual_seed(7)
            _, _, cf2, co2 = corpus.random_crops(300, L, generator=g, dtype=torch.int32)
            assert torch.equal(cf, cf2) and torch.equal(co, co2)
        pcm, lengths, cf, co = corpus.random_crops(8, 64)      # the default generator, float32
        assert pcm.dtype == torch.float32 and pcm.shape == (8, 2, 64)
        cpu = torch.Generator()
        cpu.manual_seed(3)
        pcm, lengths, cf, co = corpus.random_crops(8, 64, generator=cpu)
        assert cf.device.type == "cuda" and pcm.shape == (8, 2, 64)


def test_unchecked_crops_of_device_indices_read_nothing_back(synth):
    # torch's sync debug mode raises on every synchronising call torch itself makes (.cpu(), .item(), int(tensor), a blocking
    # copy): in "error" mode the whole step must run through
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, True)
    with pkg.Corpus([f[0] for f in files]) as corpus:
        cf, co = torch.tensor([0, 1, 4, 3], device="cuda"), torch.tensor([5, 4096, 30000, 0], device="cuda")
        want, want_len = corpus.crops(cf, co, 6000)          # (also the first call's allocations and K)
        g = torch.Generator(device="cuda")
        out = torch.empty_like(want)
        torch.cuda.synchronize()
        # the mode is honoured by this build: a read-back raises
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                want_len.cpu()
            pcm, lengths = corpus.crops(cf, co, 6000, check=False)
            pcm2, lengths2 = corpus.crops(cf, co, 6000, check=False, out=out)
            st, valid = corpus.last_status()
            r = corpus.random_crops(16, 6000, generator=g, check=False)
            with pytest.raises(RuntimeError):
                corpus.crops(cf, co, 6000, check=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(pcm, want) and torch.equal(pcm2, want) and torch.equal(lengths, want_len) and pcm2 is out
        assert bool(((st == 0) | ~valid).all()) and r[0].shape == (16, 2, 6000)


def test_two_hundred_steps_allocate_nothing_new(synth):
    import torch

    import alac.net_amd as pkg

    files = corpus_files(synth, True)
    with pkg.Corpus([f[0] for f in files]) as corpus:
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        after_two = None
        for step in range(200):
            pcm, lengths, cf, co = corpus.random_crops(32, 5000, generator=g, check=step % 2 == 0)
            plan = corpus._plan["offsets"].data_ptr()
            del pcm, lengths, cf, co
            if step == 1:
                torch.cuda.synchronize()
                after_two, plan_two = torch.cuda.memory_allocated(), plan
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == after_two and plan == plan_two      # the same plan arrays all the way


def test_sources_are_bytes_paths_and_file_objects(synth, tmp_path):
    import torch

    import alac.net_amd as pkg

    data, pcm = make_file(synth, 3, 500)
    path = tmp_path / "a.m4a"
    path.write_bytes(data)
    with open(path, "rb") as f, pkg.Corpus([data, str(path), f, memoryview(data)]) as corpus:
        assert corpus.num_frames.tolist() == [len(pcm)] * 4
        out, lengths = corpus.crops([0, 1, 2, 3], [4000] * 4, 4500, dtype=torch.int32)
        want = torch.from_numpy(pcm[4000:8500].astype(np.int32)).T.contiguous()
        assert all(torch.equal(out[b].cpu(), want) for b in range(4)) and lengths.tolist() == [4500] * 4
    corpus.close()                                   # closing twice is fine; a closed corpus refuses work
    with pytest.raises(pkg.AlacGpuError):
        corpus.crops([0], [0], 10)
    with pytest.raises(ValueError, match="source 1"):
        pkg.Corpus([data, make_file(synth, 2, 10, stereo=False)[0]])
