"""A resident corpus built from PCM on the GPU: the packet compaction (alacgpu_compact_packets_device) against its host twin,
Corpus.from_pcm against the corpus of the files save_batch writes, the round trip, ingest in batches, Corpus.save as the
checkpoint, and the memory the build takes.  Exact: nothing on this path has a tolerance."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0x5A
FRONT = 7          # bytes of the filled buffer in front of the blob's address: the blob itself is not aligned either


def expected_blob(pkg, src, sizes, slot, base, capacity, length):
    """The whole destination after a compaction of `sizes` out of the slots `src` (numpy), from compact_plan_host"""
    off, total, copied = pkg.compact_plan_host(sizes, slot, base, capacity)
    exp = np.full(length, FILL, dtype=np.uint8)
    c = np.where(np.asarray(sizes, dtype=np.uint64) <= slot, sizes, 0).astype(np.int64) * copied
    owner = np.repeat(np.arange(len(c), dtype=np.int64), c)
    within = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
    exp[off.astype(np.int64)[owner] + within] = src[owner * slot + within]
    return exp, off, total


def run_compact(torch, pkg, ctx, sizes, slot, base, capacity=None, behind=40):
    """One call over random slots into a 0x5A-filled destination that is longer than needed on both sides; asserts that the
    whole destination, the offsets and the total are the host twin's.  Returns the total."""
    dev = torch.device("cuda", 0)
    n = len(sizes)
    sizes = np.asarray(sizes, dtype=np.uint32)
    d_src = torch.randint(0, 256, (max(n * slot, 16),), dtype=torch.uint8, device=dev)
    total = pkg.compact_plan_host(sizes, slot, base, 0)[1]
    length = base + total + behind
    capacity = length if capacity is None else capacity
    raw = torch.full((FRONT + length,), FILL, dtype=torch.uint8, device=dev)
    d_blob = raw[FRONT:]
    d_sizes = torch.from_numpy(sizes.view(np.int32) if n else np.zeros(1, np.int32)).to(dev)
    d_off = torch.full((n + 2,), -2, dtype=torch.int64, device=dev)
    d_total = torch.full((3,), -2, dtype=torch.int64, device=dev)
    rc = pkg.lib().alacgpu_compact_packets_device(ctx._ctx, pkg._dp(d_src), slot, pkg._dp(d_sizes), n, pkg._dp(d_blob), base, capacity,
                                                  pkg._dp(d_off[1:]), pkg._dp(d_total[1:]), pkg._VP(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    exp, off, tot = expected_blob(pkg, d_src.cpu().numpy(), sizes, slot, base, capacity, length)
    got = raw.cpu().numpy()
    assert (got[:FRONT] == FILL).all()
    bad = np.nonzero(got[FRONT:] != exp)[0]
    assert len(bad) == 0, f"n {n} slot {slot} base {base} capacity {capacity}: {len(bad)} bytes differ, the first at {int(bad[0])}"
    assert d_off.cpu().tolist() == [-2] + off.astype(np.int64).tolist() + [-2]
    assert d_total.cpu().tolist() == [-2, tot, -2]
    return tot


def mixed_sizes(rng, n, slot):
    kinds = np.array([0, 1, 2, 3, 4, 5, 15, 16, 17, slot, slot + 1, 2 ** 32 - 1], dtype=np.uint32)
    sizes = kinds[rng.integers(0, len(kinds), n)]
    some = rng.random(n) < 0.3                      # and sizes anywhere in the slot
    sizes[some] = rng.integers(0, slot + 1, int(some.sum()))
    return sizes


def test_compaction_equals_its_host_twin():
    import torch

    import alac.net_amd as pkg

    rng = np.random.default_rng(11)
    big = pkg.encode_max_packet_bytes(4096, 16, 2)
    assert big % 16 == 0 and big > 16384
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], 0) as ctx:
        for slot in (16, 48, big):
            for n in (1, 63, 64, 65, 1025):
                for base in (range(20) if slot != big or n == 65 else (0, 13)):
                    run_compact(torch, pkg, ctx, mixed_sizes(rng, n, slot), slot, base)
            for sizes in ([slot], [slot + 1], [0], [2 ** 32 - 1], [0] * 70, [slot] * 130, [1] * 5000, [10] * 5000, [17 % slot + 1] * 3000):
                for base in (0, 5, 16):
                    run_compact(torch, pkg, ctx, sizes, slot, base)
        # every level of the scan: tiles of 2048 sizes, their sums in tiles of 2048 again, and the sums of those in ONE tile --
        # the third level exists from 2048 * 2048 + 1 packets on.  16-byte slots: 67 MB of slots, 34 MB of offsets.
        # (2049 and 2048 * 3 + 5 take two levels; everything above took one.)
        for n in (2049, 2048 * 3 + 5, 2048 * 2048 + 2048 * 5 + 77):
            run_compact(torch, pkg, ctx, rng.integers(0, 20 if n < 10000 else 7, n).astype(np.uint32), 16, 9)
        # a capacity that cuts the batch in the middle of a packet: it and all behind it are absent, offsets and total
        # complete; then the repeat with room
        for slot in (48, big):
            sizes = mixed_sizes(rng, 300, slot)
            off, total, _ = pkg.compact_plan_host(sizes, slot, 11, 0)
            counted = np.where(sizes <= slot, sizes, 0)
            p = int(np.nonzero(counted > 1)[0][150])
            for cap in (int(off[p]) + int(counted[p]) // 2, int(off[p]) + int(counted[p]) - 1, int(off[p]), 11, 5, 0):
                assert run_compact(torch, pkg, ctx, sizes, slot, 11, capacity=cap) == total
            run_compact(torch, pkg, ctx, sizes, slot, 11, capacity=11 + total)
            run_compact(torch, pkg, ctx, sizes, slot, 11)
        # n = 0: the total and nothing else
        assert run_compact(torch, pkg, ctx, np.zeros(0, np.uint32), 16, 3) == 0
        # bad arguments
        dev = torch.device("cuda", 0)
        a = torch.zeros(256, dtype=torch.uint8, device=dev)
        q = a.data_ptr()
        assert q % 16 == 0
        L, vp = pkg.lib(), pkg._VP
        good = [ctx._ctx, vp(q), 16, vp(q + 64), 1, vp(q + 128), 0, 16, vp(q + 160), vp(q + 192), None]
        assert L.alacgpu_compact_packets_device(*good) == 0
        torch.cuda.synchronize()
        for at, value in [(0, None), (1, None), (3, None), (5, None), (8, None), (9, None), (2, 24), (2, 0), (2, 8), (1, vp(q + 8)),
                          (3, vp(q + 66)), (8, vp(q + 164)), (9, vp(q + 196))]:
            args = list(good)
            args[at] = value
            assert L.alacgpu_compact_packets_device(*args) == -1, (at, value)
        torch.cuda.synchronize()


def signal(synth, C_, ss, T, seed):
    from test_encode import source

    n = -(-T // 4096)
    return source(synth, C_, ss, n, 4096, T - 4096 * (n - 1), seed=seed)


def make_batch(synth, C_, ss, lengths, seed=0, Tmax=None):
    """[F, C, Tmax] int32: the tests' signals, one file of full-scale noise (escape packets), one of zeros; frames behind a
    file's length are not part of it"""
    rng = np.random.default_rng(seed)
    Tmax = max(lengths) if Tmax is None else Tmax
    x = np.full((len(lengths), C_, Tmax), 777, np.int32)
    for f, L in enumerate(lengths):
        if f == 1:
            x[f, :, :L] = rng.integers(-(1 << (ss - 1)), 1 << (ss - 1), (C_, L))
        elif f == 2:
            x[f, :, :L] = 0
        else:
            x[f, :, :L] = signal(synth, C_, ss, L, seed * 100 + f)
    return x


def assert_same_corpus(torch, a, b):
    n = a._blob_bytes
    assert n == b._blob_bytes and torch.equal(a._blob[:n], b._blob[:n])
    assert not bool(a._blob[n:n + 16].any()) and not bool(b._blob[n:n + 16].any())
    P = len(a._host["pkt_end"])
    assert P == len(b._host["pkt_end"])
    assert torch.equal(a._pkt_offset[:P], b._pkt_offset[:P]) and torch.equal(a._pkt_size[:P], b._pkt_size[:P])
    for name in ("_pkt_end", "_file_first", "_file_cfg", "_d_num_frames"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("pkt_end", "file_first", "file_cfg", "num_frames"):
        assert np.array_equal(a._host[name], b._host[name]) and a._host[name].dtype == b._host[name].dtype, name
    assert a._gpu.cfgs.tobytes() == b._gpu.cfgs.tobytes() and a._host["cfgs"].tobytes() == b._host["cfgs"].tobytes()
    assert np.array_equal(a.num_frames, b.num_frames)
    assert (a.num_files, a.channels, a.sample_rate) == (b.num_files, b.channels, b.sample_rate)


@pytest.mark.parametrize("fl", [4096, 1000])
@pytest.mark.parametrize("C_,ss", [(1, 16), (2, 16), (1, 24), (2, 24)])
def test_a_corpus_from_pcm_is_the_corpus_of_the_saved_files(synth, C_, ss, fl):
    import torch

    import alac.net_amd as pkg

    Tmax = 3 * fl + 123
    lengths = [1, fl, fl + 1, Tmax, 2 * fl, 777]
    x = make_batch(synth, C_, ss, lengths, seed=ss + C_)
    pcm = torch.from_numpy(x).cuda()
    bufs = [io.BytesIO() for _ in lengths]
    pkg.save_batch(bufs, pcm, lengths, 48000, sample_size=ss, frame_length=fl)
    for b in bufs:
        b.seek(0)
    with pkg.Corpus(bufs) as ref, pkg.Corpus.from_pcm(pcm, lengths, 48000, sample_size=ss, frame_length=fl) as corpus:
        assert_same_corpus(torch, ref, corpus)
        assert corpus.build_stats["batches"] == 1 and corpus.sample_rate == 48000
        # the checkpoint: save writes save_batch's files, byte for byte
        again = [io.BytesIO() for _ in lengths]
        sizes = corpus.save(again)
        assert [a.getvalue() for a in again] == [b.getvalue() for b in bufs] and sizes == [len(b.getvalue()) for b in bufs]
        # round trip: crops of the whole files are the PCM up to each length, zeros behind it
        zeros = [0] * len(lengths)
        out, lens = corpus.crops(range(len(lengths)), zeros, Tmax, dtype=torch.int32)
        assert lens.cpu().tolist() == lengths
        f32 = torch.from_numpy(x.astype(np.float32) * np.float32(2.0 ** -(ss - 1))).cuda()
        with pkg.Corpus.from_pcm(f32, torch.tensor(lengths), 48000, sample_size=ss, frame_length=fl) as cf:
            assert_same_corpus(torch, corpus, cf)           # float32 as `load` returns it encodes to the same packets
            outf, _ = cf.crops(range(len(lengths)), zeros, Tmax)
        for f, L in enumerate(lengths):
            assert torch.equal(out[f, :, :L], pcm[f, :, :L]) and not bool(out[f, :, L:].any()), f
            assert torch.equal(outf[f, :, :L], f32[f, :, :L]) and not bool(outf[f, :, L:].any()), f
        # random crops equal load_batch's windows of the saved files
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        Lc = fl + 77
        got, glen, cf_, co_ = corpus.random_crops(40, Lc, generator=g, dtype=torch.int32)
        files, offs = cf_.cpu().tolist(), co_.cpu().tolist()
        want, wlen, _ = pkg.load_batch([bufs[f].getvalue() for f in files], dtype=torch.int32, max_frames=Lc, frame_offsets=offs)
        assert glen.cpu().tolist() == wlen.tolist()
        assert torch.equal(got[:, :, :want.shape[2]], want) and not bool(got[:, :, want.shape[2]:].any())


def test_ingest_in_batches(synth):
    import torch

    import alac.net_amd as pkg

    shapes = [([5000, 4096, 17], 6000), ([1, 8193], 9000), ([30000, 12000, 4097, 25000, 29999], 30000)]
    batches = [(make_batch(synth, 2, 16, lens, seed=40 + i, Tmax=T), lens) for i, (lens, T) in enumerate(shapes)]
    lengths = sum((lens for _, lens in batches), [])
    whole = np.zeros((len(lengths), 2, 30000), np.int32)
    f = 0
    for x, lens in batches:
        whole[f:f + len(lens), :, :x.shape[2]] = x
        f += len(lens)
    gen = ((torch.from_numpy(x).cuda(), lens) for x, lens in batches)        # an iterator: nothing holds all the PCM
    with pkg.Corpus.from_pcm(gen, sample_rate=44100) as parts, \
            pkg.Corpus.from_pcm(torch.from_numpy(whole).cuda(), lengths, 44100) as one:
        assert_same_corpus(torch, one, parts)
        st = parts.build_stats
        assert st["batches"] == 3 and st["grown"] >= 1 and st["compactions"] == st["batches"] + st["grown"]
        assert st["capacity"] >= parts._blob_bytes and parts._blob.numel() == st["capacity"] + 64
        out, lens = parts.crops(range(len(lengths)), [0] * len(lengths), 30000, dtype=torch.int32)
        assert lens.cpu().tolist() == lengths
        for f, L in enumerate(lengths):
            assert np.array_equal(out[f, :, :L].cpu().numpy(), whole[f, :, :L]) and not bool(out[f, :, L:].any())
    with pytest.raises(ValueError, match="batch 1"):     # every batch has the first's channel count
        pkg.Corpus.from_pcm([(torch.zeros((1, 2, 50), dtype=torch.int32).cuda(), [50]),
                             (torch.zeros((1, 1, 50), dtype=torch.int32).cuda(), [50])], sample_rate=44100)


def test_save_checkpoints_a_corpus_of_files(synth, tmp_path):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import container
    from alac.net_amd.synth import m4a
    from test_corpus import corpus_files

    files = [f[0] for f in corpus_files(synth, True)]
    # ... and a file of 16384-frame packets with a short last one, its Rice parameters not the encoder's
    d = synth.packet_descs(3, sample_size=16, stereo=1, pred_order=8, max_samples_per_frame=16384, rice_history_mult=36, rice_kmodifier=12)
    d["n"][:] = [16384, 16384, 5]
    b = synth.make_batch(d, synth.default_signal(3), want_pcm=True)
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    files.append(m4a.write_m4a(packets, [16384, 16384, 5], frame_len=16384, sample_size=16, channels=2, sample_rate=44100,
                               pb=36, kb=12))
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"in_{i}.m4a"))
        open(paths[-1], "wb").write(data)
    outs = [str(tmp_path / f"out_{i}.m4a") for i in range(len(files) - 1)] + [io.BytesIO()]
    with pkg.Corpus(paths) as corpus:
        sizes = corpus.save(outs)
        with pytest.raises(ValueError):
            corpus.save(outs[:2])
    saved = [open(o, "rb").read() for o in outs[:-1]] + [outs[-1].getvalue()]
    assert sizes == [len(s) for s in saved]
    for i, (data, back) in enumerate(zip(files, saved)):
        t, u = container.packet_table(data), container.packet_table(back)
        assert np.array_equal(t["sizes"], u["sizes"]) and np.array_equal(t["durations"], u["durations"]), i
        assert t["cfg"].tobytes() == u["cfg"].tobytes() and t["blob"].tobytes() == u["blob"].tobytes(), i
        assert (t["sample_rate"], t["num_channels"], t["sample_size"]) == (u["sample_rate"], u["num_channels"], u["sample_size"])
    with pkg.Corpus(saved) as again, pkg.Corpus(files) as ref:
        assert_same_corpus(torch, ref, again)


def tone(torch, F, C_, T, seed):
    """[F, C, T] int32 on the device: a few sines and a little noise, generated there"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float32)
    w = torch.rand((F, C_, 1), generator=g, device="cuda") * 0.05 + 0.01
    x = 9000 * torch.sin(t * w) + 3000 * torch.sin(t * w * 3.7) + 40 * torch.randn((F, C_, T), generator=g, device="cuda")
    return x.to(torch.int32)


def test_no_tensor_grows_with_the_packet_bytes():
    """A condition, not a measurement: around a from_pcm of 320 MB of PCM the allocator's peak, less the PCM, stays below the
    blob, one batch's slot buffer and one more blob (the copy while it grows) plus a fixed 64 MiB; a gather with int64
    temporaries per packet byte breaks that by an order of magnitude.  The same for save_batch, whose blob is the packets'
    bytes."""
    import torch

    import alac.net_amd as pkg

    F, C_, T = 32, 2, 1250000
    pcm = tone(torch, F, C_, T, 1)
    lengths = [T - 1000 * f for f in range(F)]
    slots = sum(-(-L // 4096) for L in lengths) * pkg.encode_max_packet_bytes(4096, 16, C_)
    fixed = 64 << 20
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert before >= pcm.numel() * 4
    with pkg.Corpus.from_pcm(pcm, lengths, 44100) as corpus:
        peak = torch.cuda.max_memory_allocated() - before
        blob = corpus._blob.numel()
        print(f"from_pcm: peak {peak} blob {blob} slots {slots} packets' bytes {corpus._blob_bytes} stats {corpus.build_stats}")
        assert corpus._blob_bytes > 50 << 20
        assert peak <= blob + slots + blob + fixed
    del corpus
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sink = [io.BytesIO() for _ in range(F)]
    sizes = pkg.save_batch(sink, pcm, lengths, 44100)
    peak = torch.cuda.max_memory_allocated() - before
    blob = sum(sizes)                  # (a little more than the packets' bytes: the files' tables)
    print(f"save_batch: peak {peak} blob {blob} slots {slots}")
    assert peak <= blob + slots + blob + fixed
