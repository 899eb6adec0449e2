"""A corpus with a host tier on the GPU: the staging kernel (alacgpu_stage_packets_device) against its host twin, and crops of
a corpus that lies partly or wholly in page-locked host memory bit-equal to those of the resident one -- exact: nothing on
this path has a tolerance."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0x5A
GUARD = 64          # bytes in front of and behind the staging blob; elements around the two small outputs


def round16(x):
    return (int(x) + 15) // 16 * 16


def run_stage(torch, pkg, ctx, src, lo_bytes, hi_bytes, hi_kind, src_offset, sizes, capacity):
    """alacgpu_stage_packets_device over the source space `src` (numpy uint8 of lo_bytes + hi_bytes bytes; the second part in
    device memory or in page-locked host memory) into a staging blob with GUARD bytes of FILL around it and FILL inside; the
    offsets and the total are guarded the same way.  Compares everything with stage_plan_host and returns the total."""
    dev = torch.device("cuda", 0)
    n = len(sizes)
    part = lambda a: np.concatenate([a, np.zeros(round16(len(a)) - len(a) + 16, np.uint8)])
    d_lo = torch.from_numpy(part(src[:lo_bytes])).to(dev) if lo_bytes else None
    pinned = None
    if not hi_bytes:
        hi = None
    elif hi_kind == "device":
        hi = torch.from_numpy(part(src[lo_bytes:])).to(dev)
    else:
        pinned = pkg.PinnedBuffer(round16(hi_bytes) + 16, np.uint8)
        pinned.array[:] = part(src[lo_bytes:])
        hi = pinned.array.ctypes.data
    try:
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if len(a) else np.zeros(1, dt)).to(dev)
        d_off, d_size = up(np.asarray(src_offset, dtype=np.uint64), np.int64), up(np.asarray(sizes, dtype=np.uint32), np.int32)
        want_off, want_total, copied = pkg.stage_plan_host(src_offset, sizes, lo_bytes, hi_bytes, capacity)
        room = round16(min(capacity, want_total)) + 4096           # (the fill behind the capacity is looked at too)
        raw = torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device=dev)
        raw_off = torch.full(((n + 2 * GUARD) * 8,), FILL, dtype=torch.uint8, device=dev).view(torch.int64)
        raw_total = torch.full(((1 + 2 * GUARD) * 8,), FILL, dtype=torch.uint8, device=dev).view(torch.int64)
        stage, so, total = raw[GUARD:GUARD + room], raw_off[GUARD:GUARD + n], raw_total[GUARD:GUARD + 1]
        assert stage.data_ptr() % 16 == 0
        ctx.stage_packets_device(d_lo, lo_bytes, hi, hi_bytes, d_off, d_size, n, stage, capacity, so, total,
                                 stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for r, m in ((raw_off, n), (raw_total, 1)):
            assert bool((torch.cat([r[:GUARD], r[GUARD + m:]]).view(torch.uint8) == FILL).all()), "a store outside an output array"
        assert int(total[0]) == want_total
        assert np.array_equal(so.cpu().numpy().view(np.uint64)[:n], want_off)
        got = raw.cpu().numpy()
        # the blob as it has to be: FILL, and the copied packets' bytes; the bytes up to a packet's round-up may be anything
        want = np.full(len(got), FILL, np.uint8)
        known = np.ones(len(got), bool)
        for j in np.nonzero(copied)[0]:
            o, s, a = int(want_off[j]) + GUARD, int(sizes[j]), int(src_offset[j])
            assert o - GUARD + round16(s) <= capacity
            want[o:o + s] = src[a:a + s]
            known[o + s:o - GUARD + round16(s) + GUARD] = False
        bad = np.nonzero((got != want) & known)[0]
        assert len(bad) == 0, (len(bad), bad[:5] - GUARD, capacity, want_total)
        assert (got[GUARD + min(want_total, capacity):] == FILL).all() and (got[:GUARD] == FILL).all()
        return want_total, int(copied.sum())
    finally:
        if pinned is not None:
            pinned.close()


def stage_plans(rng, lo_bytes, hi_bytes):
    """(src_offset, sizes) of plans of every kind the kernel meets"""
    end = lo_bytes + hi_bytes
    kinds = [0, 1, 15, 16, 17, 16400]
    # adversarial: every size at every source alignment in both parts, touching both ends of each part, straddling lo_bytes,
    # past the end, the largest values, duplicates of one packet
    adv = []
    for s in kinds:
        for base in (0, lo_bytes) if hi_bytes else (0,):
            limit = (lo_bytes if base == 0 and lo_bytes else end) - base
            adv += [(base + a, s) for a in range(16) if a + s <= limit]
            adv += [(base + limit - s, s)] if s <= limit else []                  # ends with its part
            adv += [(base + limit - s + 1, s)] if s <= limit else []              # one byte too far: straddles or leaves the space
        adv += [(end, s), (end + 1, s), (2 ** 64 - 1, s), (2 ** 63, s)]
    if lo_bytes and hi_bytes:
        adv += [(lo_bytes - 1, 2), (lo_bytes - 8, 16), (max(lo_bytes - 16399, 0), 16400), (0, 2 ** 32 - 1)]
    adv += [(end // 2 + 3, 16400 if end > 40000 else 17)] * 5
    adv += [(7, 1000)] * 3 if lo_bytes + hi_bytes > 2000 else []
    yield "adversarial", adv
    # random: n above one scan tile and a multiple of no tile
    n = 2 * 2048 + 777
    sizes = rng.choice(kinds + [100, 2000, 11000], n)
    offs = rng.integers(0, end + 300, n)
    yield "random", list(zip(offs.tolist(), sizes.tolist()))
    # a plan as the planner leaves it: runs of packets back to back, padding entries (offset 0, size 0) behind each
    plan, at = [], 0
    for crop in range(300):
        at = int(rng.integers(0, max(end - 60000, 1)))
        for k in range(int(rng.integers(0, 6))):
            s = int(rng.integers(1, 12000))
            plan.append((at, s))
            at += s
        plan += [(0, 0)] * int(rng.integers(0, 4))
    yield "plan", plan


@pytest.mark.parametrize("hi_kind", ["device", "pinned"])
def test_staging_equals_its_host_twin(hi_kind):
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(23)
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        for lo_bytes, hi_bytes in ((70003, 90005), (0, 100001), (100000, 0), (33, 20)):
            src = rng.integers(0, 256, lo_bytes + hi_bytes, dtype=np.uint8)
            for name, plan in stage_plans(rng, lo_bytes, hi_bytes):
                off = np.array([p[0] for p in plan], dtype=np.uint64)
                size = np.array([p[1] for p in plan], dtype=np.uint32)
                total, n_copied = run_stage(torch, pkg, ctx, src, lo_bytes, hi_bytes, hi_kind, off, size, 2 ** 40)
                assert name != "random" or (lo_bytes + hi_bytes < 1000) or (total > 10 ** 6 and n_copied > 1000)
                # the capacity: exactly at the total, one below, in the middle (a multiple of 16 or not), next to nothing
                for cap in (total, total - 1, total // 2 + 5, (total // 32) * 16, 16, 15, 0):
                    if cap >= 0:
                        run_stage(torch, pkg, ctx, src, lo_bytes, hi_bytes, hi_kind, off, size, cap)
        # no packets: the total and nothing else
        dev = torch.device("cuda", 0)
        t = torch.full((16,), -1, dtype=torch.int64, device=dev)
        ctx.stage_packets_device(None, 0, None, 0, None, None, 0, None, 0, None, t[8:9], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert t.tolist() == [-1] * 8 + [0] + [-1] * 7


def test_staging_refuses_bad_arguments_before_any_launch():
    import torch

    import alac.net_amd as pkg

    dev = torch.device("cuda", 0)
    L_ = pkg.lib()
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        src = torch.zeros(4096, dtype=torch.uint8, device=dev)
        off = torch.zeros(8, dtype=torch.int64, device=dev)
        size = torch.full((8,), 16, dtype=torch.int32, device=dev)
        stage = torch.full((4096,), FILL, dtype=torch.uint8, device=dev)
        so = torch.full((8,), -1, dtype=torch.int64, device=dev)
        total = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ordinary = np.zeros(4096 + 16, np.uint8)
        ordinary_at = (ordinary.ctypes.data + 15) // 16 * 16          # memory that is neither device memory nor page-locked
        P, V = pkg._dp, pkg._VP

        def call(**kw):
            a = dict(ctx=ctx._ctx, lo=P(src), lo_bytes=2048, hi=V(src.data_ptr() + 2048), hi_bytes=2048, off=P(off), size=P(size), n=8,
                     stage=P(stage), cap=4096, so=P(so), total=P(total))
            a.update(kw)
            return L_.alacgpu_stage_packets_device(a["ctx"], a["lo"], a["lo_bytes"], a["hi"], a["hi_bytes"], a["off"], a["size"], a["n"],
                                                   a["stage"], a["cap"], a["so"], a["total"], V(torch.cuda.current_stream().cuda_stream))

        plus = lambda t, k: V(t.data_ptr() + k)
        for kw in (dict(ctx=None), dict(off=None), dict(size=None), dict(stage=None), dict(so=None), dict(total=None),
                   dict(lo=None), dict(hi=None), dict(lo=plus(src, 8)), dict(hi=plus(src, 2056)), dict(stage=plus(stage, 8)),
                   dict(size=plus(size, 2)), dict(off=plus(off, 4)), dict(so=plus(so, 4)), dict(total=plus(total, 4)),
                   dict(hi=V(ordinary_at)), dict(n=0, total=plus(total, 4)), dict(lo_bytes=2 ** 64 - 1)):
            assert call(**kw) == -1, kw
        torch.cuda.synchronize()
        assert bool((stage == FILL).all()) and so.tolist() == [-1] * 8 and total.tolist() == [-1]      # nothing was enqueued
        # a NULL base with no bytes is fine, and so is the call itself
        assert call(lo=None, lo_bytes=0, hi=P(src), hi_bytes=4096) == 0
        assert call() == 0
        torch.cuda.synchronize()
        assert so.tolist() == [16 * j for j in range(8)] and total.tolist() == [128] and bool((stage[128:] == FILL).all())


def file_bytes_of(files):
    from alac.net_amd import container

    return [int(container.header_table(f)["sizes"].sum()) for f in files]


def splits_of(files):
    """hbm_bytes that put everything on the host, cut the corpus in the middle (one byte more than two files: the third is not
    split), and keep every file but the last in HBM"""
    n = file_bytes_of(files)
    return [(0, 0), (n[0] + n[1] + 1, 2), (sum(n) - 1, len(n) - 1)]


@pytest.mark.parametrize("stereo", [True, False])
def test_crops_of_a_tiered_corpus_equal_those_of_the_resident_one(synth, stereo):
    import torch

    import alac.net_amd as pkg
    from test_corpus import corpus_files, some_crops

    files = corpus_files(synth, stereo)
    data = [f[0] for f in files]
    sizes = file_bytes_of(data)
    rng = np.random.default_rng(4)
    with pkg.Corpus(data) as resident:
        assert resident.tier_bytes == (sum(sizes), 0)
        with pkg.Corpus(data, hbm_bytes=sum(sizes)) as same, pkg.Corpus(data, hbm_bytes=10 ** 12) as same2:
            # nothing ends up on the host: exactly the resident corpus, and its code path
            for c in (same, same2):
                assert c.tier_bytes == (sum(sizes), 0) and c._pinned is None
                pcm, lengths = c.crops([0, 4], [5, 100], 3000, dtype=torch.int32)
                want, want_len = resident.crops([0, 4], [5, 100], 3000, dtype=torch.int32)
                assert torch.equal(pcm, want) and torch.equal(lengths, want_len) and c._stage is None
        for h, on_device in splits_of(data):
            with pkg.Corpus(data, hbm_bytes=h) as corpus:
                assert corpus.tier_bytes == (sum(sizes[:on_device]), sum(sizes[on_device:])) and corpus.tier_bytes[1] > 0
                assert corpus.num_files == 5 and corpus.num_frames.tolist() == resident.num_frames.tolist()
                for L in (1, 3000, 2 * 4096 + 1):
                    crops = some_crops(files, L, rng)        # offset 0, the last frame, the end itself, packet boundaries
                    cf, co = [c[0] for c in crops], [c[1] for c in crops]
                    assert corpus.stage_bytes_per_crop(L) == pkg.stage_bytes_per_crop(
                        resident._host["pkt_size"], resident._host["pkt_end"], resident._host["file_first"], L) > 0
                    for dtype in (torch.float32, torch.int32):
                        want, want_len = resident.crops(cf, co, L, dtype=dtype)
                        for k, (a, b_) in enumerate(((cf, co), (np.array(cf, dtype=np.int32), np.array(co, dtype=np.uint64)),
                                                     (torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")),
                                                     (torch.tensor(cf, device="cuda", dtype=torch.int32), torch.tensor(co, device="cuda")))):
                            out = None
                            if k % 2:
                                out = torch.full((len(crops), corpus.channels, L), 12345, dtype=dtype, device="cuda")
                            pcm, lengths = corpus.crops(a, b_, L, dtype=dtype, out=out)
                            assert out is None or pcm is out
                            assert pcm.dtype == dtype and lengths.dtype == torch.int64 and lengths.device.type == "cuda"
                            assert torch.equal(lengths, want_len) and torch.equal(pcm, want), (h, L, dtype, k)
                    assert corpus._stage.numel() >= len(crops) * corpus.stage_bytes_per_crop(L) + 64
                # nothing to decode
                pcm, lengths = corpus.crops([], [], 100)
                assert pcm.shape == (0, corpus.channels, 100) and lengths.shape == (0,)
                pcm, lengths = corpus.crops([0, 1], [5, 0], 0, dtype=torch.int32)
                assert pcm.shape == (2, corpus.channels, 0) and lengths.tolist() == [0, 0]
                with pytest.raises(ValueError):
                    corpus.crops([5], [0], 10)
                # device indices outside the corpus: a length code, a row of zeros, and a ValueError when checked
                a, b_ = torch.tensor([0, 7, 1, 4], device="cuda"), torch.tensor([3, 0, 10 ** 9, 7], device="cuda")
                pcm, lengths = corpus.crops(a, b_, 50, dtype=torch.int32, check=False)
                want, want_len = resident.crops(a, b_, 50, dtype=torch.int32, check=False)
                assert lengths.tolist() == [50, -1, -1, 50] and torch.equal(pcm, want) and not pcm[1:3].any() and pcm[3].any()
                with pytest.raises(ValueError, match="crop 1"):
                    corpus.crops(a, b_, 50)
                # one seeded generator on both
                for L in (100, 5000, 40000):
                    g = torch.Generator(device="cuda")
                    g.manual_seed(7)
                    pcm, lengths, cf, co = corpus.random_crops(300, L, generator=g, dtype=torch.int32)
                    g.manual_seed(7)
                    want, want_len, cf2, co2 = resident.random_crops(300, L, generator=g, dtype=torch.int32)
                    assert torch.equal(cf, cf2) and torch.equal(co, co2) and torch.equal(lengths, want_len) and torch.equal(pcm, want)
                    assert len(set(cf.tolist())) == 5
    for bad in (-1, 1.5, "7"):
        with pytest.raises(ValueError):
            pkg.Corpus(data, hbm_bytes=bad)


def test_an_unchecked_tiered_step_reads_nothing_back(synth):
    import torch

    import alac.net_amd as pkg
    from test_corpus import corpus_files

    files = corpus_files(synth, True)
    data = [f[0] for f in files]
    with pkg.Corpus(data) as resident, pkg.Corpus(data, hbm_bytes=splits_of(data)[1][0]) as corpus:
        cf, co = torch.tensor([0, 1, 4, 3], device="cuda"), torch.tensor([5, 4096, 30000, 0], device="cuda")
        want, want_len = resident.crops(cf, co, 6000)
        first, _ = corpus.crops(cf, co, 6000)                # (also the first call's allocations, K and S)
        corpus.random_crops(16, 6000, check=False)
        g = torch.Generator(device="cuda")
        out = torch.empty_like(want)
        torch.cuda.synchronize()
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
        assert torch.equal(first, want) and torch.equal(pcm, want) and torch.equal(pcm2, want) and torch.equal(lengths, want_len)
        assert pcm2 is out and bool(((st == 0) | ~valid).all()) and r[0].shape == (16, 2, 6000)


def test_a_corrupt_packet_in_the_host_tier_is_named_as_in_the_resident_corpus(synth):
    import torch

    import alac.net_amd as pkg
    from test_corpus import make_file
    from test_load_window import corrupt

    data, pcm = make_file(synth, 6, 2000)
    good, pcm_good = make_file(synth, 4, 4096, seed=9)
    bad = corrupt(data, 2)                     # frames 8192 .. 12288 of source 1 do not decode
    n_good = file_bytes_of([good])[0]
    with pkg.Corpus([good, bad]) as resident:
        for h in (n_good, 0):
            with pkg.Corpus([good, bad], hbm_bytes=h) as corpus:
                assert corpus.tier_bytes[0] == h and corpus.tier_bytes[1] > 0
                for cf, co, L in (([0, 1], [0, 8191], 2), ([1, 0, 1], [12287, 5, 0], 10), ([0, 0, 1], [0, 1, 4000], 8000)):
                    for dev_idx in (False, True):
                        a, b_ = (torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")) if dev_idx else (cf, co)
                        with pytest.raises(pkg.AlacGpuError) as want:
                            resident.crops(a, b_, L)
                        with pytest.raises(pkg.AlacGpuError) as got:
                            corpus.crops(a, b_, L)
                        assert str(got.value) == str(want.value) and "(source 1), packet 2 does not decode: status" in str(got.value)
                # crops around the packet are right, checked
                out, _ = corpus.crops([0, 1, 1, 1], [100, 0, 12288, 100], 8000, dtype=torch.int32)
                want, _ = resident.crops([0, 1, 1, 1], [100, 0, 12288, 100], 8000, dtype=torch.int32)
                assert torch.equal(out, want)
                # unchecked: the same zeros, the same statuses
                out, lengths = corpus.crops([0, 1], [0, 4000], 10000, dtype=torch.int32, check=False)
                st, valid = corpus.last_status()
                want, want_len = resident.crops([0, 1], [0, 4000], 10000, dtype=torch.int32, check=False)
                want_st, want_valid = resident.last_status()
                assert torch.equal(out, want) and torch.equal(lengths, want_len)
                assert torch.equal(st, want_st) and torch.equal(valid, want_valid) and st[6].item() in (3, 6)
                row = pcm[4000:14000].astype(np.int32).copy()
                row[8192 - 4000:12288 - 4000] = 0
                assert torch.equal(out[1].cpu(), torch.from_numpy(row).T.contiguous())


def test_save_and_close_of_a_tiered_corpus(synth):
    import torch

    import alac.net_amd as pkg
    from test_corpus import corpus_files

    files = corpus_files(synth, True)
    data = [f[0] for f in files]
    with pkg.Corpus(data) as resident:
        sinks = [io.BytesIO() for _ in data]
        resident.save(sinks)
        saved = [s.getvalue() for s in sinks]
    for h, _ in splits_of(saved):
        corpus = pkg.Corpus(saved, hbm_bytes=h)
        sinks = [io.BytesIO() for _ in saved]
        lengths = corpus.save(sinks)
        assert [s.getvalue() for s in sinks] == saved and lengths == [len(s) for s in saved]     # byte for byte the source files
        # from the original files too: what the resident corpus writes
        with pkg.Corpus(data, hbm_bytes=h) as again:
            sinks = [io.BytesIO() for _ in saved]
            again.save(sinks)
            assert [s.getvalue() for s in sinks] == saved
        assert corpus._pinned is not None
        corpus.close()
        assert corpus._pinned is None and corpus._stage is None and corpus._blob is None      # the page-locked buffer is gone
        corpus.close()                                                                        # twice is fine
        with pytest.raises(pkg.AlacGpuError):
            corpus.crops([0], [0], 10)
        with pytest.raises(pkg.AlacGpuError):
            corpus.save([io.BytesIO() for _ in saved])
    # a constructor that fails behind the allocation of the host blob frees it
    mono = __import__("test_corpus").make_file(synth, 2, 10, stereo=False)[0]
    with pytest.raises(ValueError, match="source 5"):
        pkg.Corpus(data + [mono], hbm_bytes=0)
    torch.cuda.synchronize()
