"""The host side of alac.Corpus: corpus_plan_host (the crop planner's specification) against window_plan crop by crop, the
K(L) bound against every offset of small tables, the resident tables of a corpus, and the new entry point's declaration.
CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-made duration tables: regular with a short last packet, one packet, zero-duration packets between and around others,
# irregular, the longest frame, a duration above it (the skip clamp), no frames at all, no packets
TABLES = [
    [4096, 4096, 4096, 1234],
    [17],
    [0, 3, 0, 0, 5, 16384, 0, 2, 0],
    [4096, 4096, 1000, 4096, 1234],
    [1, 17, 1000, 16384, 1, 1, 4096],
    [4096, 20000, 4096, 4096],
    [0, 0],
    [],
]


def tables_of(duration_lists, rng=None):
    """The resident tables of files with these durations (sizes and cfg rows made up: the plan only copies them)"""
    rng = rng or np.random.default_rng(3)
    counts = [len(d) for d in duration_lists]
    file_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    pkt_end = np.concatenate([np.cumsum(np.asarray(d, dtype=np.int64)) for d in duration_lists] + [np.zeros(0, np.int64)])
    pkt_size = rng.integers(0, 5000, int(file_first[-1])).astype(np.uint32)
    pkt_offset = np.concatenate([[0], np.cumsum(pkt_size.astype(np.uint64))[:-1]]).astype(np.uint64)[:len(pkt_size)]
    file_cfg = (np.arange(len(duration_lists)) % 3).astype(np.uint16)
    return dict(pkt_offset=pkt_offset, pkt_size=pkt_size, pkt_end=pkt_end.astype(np.uint64), file_first=file_first, file_cfg=file_cfg)


def edge_offsets(durations):
    T = int(np.sum(durations))
    bounds = np.concatenate([[0], np.cumsum(np.asarray(durations, dtype=np.int64))])
    near = {int(b) + d for b in bounds for d in (-1, 0, 1)} | {0, 1, T - 1, T}
    return sorted(o for o in near if 0 <= o <= T)


def check_against_window_plan(pkg, duration_lists, crops, L, K, stride=None):
    """corpus_plan_host over `crops` = [(file, offset)], and every crop's entries against window_plan of its file"""
    tb = tables_of(duration_lists)
    stride = 2 * L if stride is None else stride
    cf = np.array([c[0] for c in crops], dtype=np.uint32)
    co = np.array([c[1] for c in crops], dtype=np.uint64)
    off, size, cfg, first, frames, skip, lengths = pkg.corpus_plan_host(
        tb["pkt_offset"], tb["pkt_size"], tb["pkt_end"], tb["file_first"], tb["file_cfg"], cf, co, L, K, stride)
    assert [a.dtype for a in (off, size, cfg, first, frames, skip, lengths)] == \
        [np.uint64, np.uint32, np.uint16, np.uint64, np.uint32, np.uint32, np.int64]
    assert all(len(a) == len(crops) * K for a in (off, size, cfg, first, frames, skip)) and len(lengths) == len(crops)
    for b, (f, o) in enumerate(crops):
        j = slice(b * K, (b + 1) * K)
        d = np.asarray(duration_lists[f], dtype=np.int64) if f < len(duration_lists) else None
        if d is None or o > int(d.sum()):
            assert lengths[b] == -1
            n = 0
        else:
            want_len = min(L, int(d.sum()) - o)
            dst_first = np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.int64) if len(d) else np.zeros(0, np.int64)
            p0, p1, w_first, w_frames, w_skip = pkg.window_plan(dst_first, d, o, want_len)
            if p1 - p0 > K:
                assert lengths[b] == -2
                n = 0
            else:
                assert lengths[b] == want_len, (f, o, L)
                n = p1 - p0
                g = int(tb["file_first"][f]) + p0
                assert np.array_equal(off[j][:n], tb["pkt_offset"][g:g + n]) and np.array_equal(size[j][:n], tb["pkt_size"][g:g + n])
                assert (cfg[j][:n] == tb["file_cfg"][f]).all()
                assert np.array_equal(first[j][:n].astype(np.int64), b * stride + w_first), (f, o, L)
                assert np.array_equal(frames[j][:n].astype(np.int64), w_frames), (f, o, L)
                assert np.array_equal(skip[j][:n].astype(np.int64), np.minimum(w_skip, 16384)), (f, o, L)
        # padding: the switched-off cfg and zeros elsewhere
        assert (cfg[j][n:] == 0xFFFF).all()
        for a in (off, size, first, frames, skip):
            assert (a[j][n:] == 0).all()
    return lengths


def test_plan_equals_window_plan_on_hand_made_tables():
    import alac.net_amd as pkg

    for L in (0, 1, 2, 17, 4095, 4096, 4097, 3 * 4096, 20000, 40000):
        K = max(pkg.entries_per_crop(tables_of(TABLES)["pkt_end"], tables_of(TABLES)["file_first"], L), 1)
        crops = [(f, o) for f, d in enumerate(TABLES) for o in edge_offsets(d)]
        lengths = check_against_window_plan(pkg, TABLES, crops, L, K)
        assert (lengths >= 0).all()          # K(L) is enough for every one of them
    # a duration above 16384: the skip is clamped, the frames are not
    tb = tables_of(TABLES)
    f = 5
    out = pkg.corpus_plan_host(tb["pkt_offset"], tb["pkt_size"], tb["pkt_end"], tb["file_first"], tb["file_cfg"],
                               [f], [4096 + 17000], 100, 2, 200)
    assert out[5][:2].tolist() == [16384, 0] and out[4][:2].tolist() == [100, 0] and out[2][:2].tolist() == [f % 3, 0xFFFF]
    assert out[6].tolist() == [100]


def test_plan_on_files_like_the_loaders_tests(synth):
    # mixed packet counts, short last packets, a one-packet file: built as tests/test_load_window.py builds its files, and read
    # back through the demuxer
    import alac.net_amd as pkg
    from alac.net_amd import container
    from alac.net_amd.synth import m4a

    files = []
    for n_packets, last, ss in ((3, 100, 16), (5, 4000, 24), (1, 17, 16), (4, 4096, 24)):
        d = synth.packet_descs(n_packets, sample_size=ss, stereo=1, pred_order=8 if ss == 16 else 16)
        d["n"][-1] = last
        b = synth.make_batch(d, synth.default_signal(n_packets))
        packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
        files.append(m4a.write_m4a(packets, [int(x) for x in d["n"]], sample_size=ss, channels=2, sample_rate=44100))
    heads = [container.packet_table(f) for f in files]
    tb = pkg.corpus_tables(heads)
    durations = [h["durations"].tolist() for h in heads]
    assert tb["num_frames"].tolist() == [2 * 4096 + 100, 4 * 4096 + 4000, 17, 4 * 4096]
    rng = np.random.default_rng(8)
    for L in (0, 1, 4096, 6000, 3 * 4096 + 5):
        K = max(pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L), 1)
        crops = [(f, o) for f, d in enumerate(durations) for o in edge_offsets(d)]
        crops += [(int(f), int(rng.integers(0, tb["num_frames"][f] + 1))) for f in rng.integers(0, 4, 100)]
        crops += [(4, 0), (0, int(tb["num_frames"][0]) + 1), (2 ** 32 - 1, 0), (1, 2 ** 63 + 5)]     # outside the corpus: -1
        lengths = check_against_window_plan(pkg, durations, crops, L, K)
        assert lengths[-4:].tolist() == [-1] * 4 and (lengths[:-4] >= 0).all()
    # the real tables: offsets and sizes are the demuxer's, file after file
    base = 0
    for f, h in enumerate(heads):
        g0, g1 = int(tb["file_first"][f]), int(tb["file_first"][f + 1])
        assert np.array_equal(tb["pkt_offset"][g0:g1], h["offsets"] + np.uint64(base)) and np.array_equal(tb["pkt_size"][g0:g1], h["sizes"])
        assert int(tb["file_base"][f]) == base
        base += int(h["sizes"].sum())
    assert tb["blob_bytes"] == base == int(tb["file_base"][-1])


def test_a_k_that_is_too_small_is_a_length_code_and_padding():
    import alac.net_amd as pkg

    crops = [(0, 0), (0, 4095), (3, 100), (1, 3)]
    lengths = check_against_window_plan(pkg, TABLES, crops, 3 * 4096, 2)
    assert lengths.tolist() == [-2, -2, -2, 14]
    lengths = check_against_window_plan(pkg, TABLES, crops, 3 * 4096, 4)
    assert lengths.tolist() == [3 * 4096, 3 * 4096 + 1234 - 4095, 3 * 4096, 14]


def brute_force_k(durations, L):
    import alac.net_amd as pkg

    d = np.asarray(durations, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.int64) if len(d) else np.zeros(0, np.int64)
    T = int(d.sum())
    best = 0
    for o in range(T + 1):
        p0, p1 = pkg.window_plan(first, d, o, min(L, T - o))[:2]
        best = max(best, p1 - p0)
    return best


def test_entries_per_crop_is_the_exact_maximum():
    import alac.net_amd as pkg

    rng = np.random.default_rng(21)
    for trial in range(60):
        files = [rng.integers(0, 8, int(rng.integers(0, 40))).tolist() for _ in range(int(rng.integers(1, 5)))]
        tb = tables_of(files, rng)
        for L in (1, 2, 3, 5, 8, 13, 40, 1000):
            want = max(brute_force_k(d, L) for d in files)     # every file, every offset: none needs more, one needs as many
            assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L) == want, (files, L)
        assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], 0) == 0
    # one frame length: ceil((L - 1) / fl) + 1 when the file is long enough
    for fl, n, last in ((4096, 40, 4096), (4096, 40, 7), (1024, 100, 1000), (5, 50, 5), (1, 30, 1)):
        tb = tables_of([[fl] * (n - 1) + [last]])
        for L in (1, 2, fl - 1, fl, fl + 1, fl + 2, 2 * fl, 2 * fl + 1, 2 * fl + 2, 10 * fl + 3):
            if L >= 1 and L + 2 * fl < fl * (n - 1):
                assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L) == -(-(L - 1) // fl) + 1, (fl, L)
    assert pkg.entries_per_crop(np.zeros(0, np.uint64), [0, 0], 5) == 0


def head(pkg, durations, sample_size=16, channels=2, rate=44100, frame_length=4096):
    return dict(sizes=np.full(len(durations), 100, np.uint32), durations=np.asarray(durations, dtype=np.int64),
                cfg=pkg.make_cfgs([(frame_length, sample_size, 40, 10, 14, channels)]), num_channels=channels, sample_rate=rate)


def test_corpus_tables_share_cfg_rows_and_refuse_mixed_streams():
    import alac.net_amd as pkg

    heads = [head(pkg, [4096, 4096, 10]), head(pkg, [4096], 24), head(pkg, []), head(pkg, [4096, 1], 16), head(pkg, [7, 0, 9], 24)]
    tb = pkg.corpus_tables(heads)
    assert tb["file_first"].tolist() == [0, 3, 4, 4, 6, 9] and tb["file_first"].dtype == np.uint32
    assert tb["pkt_end"].tolist() == [4096, 8192, 8202, 4096, 4096, 4097, 7, 7, 16] and tb["pkt_end"].dtype == np.uint64
    assert tb["pkt_offset"].tolist() == [100 * i for i in range(9)] and tb["pkt_offset"].dtype == np.uint64
    assert tb["num_frames"].tolist() == [8202, 4096, 0, 4097, 16] and tb["blob_bytes"] == 900
    assert (tb["channels"], tb["sample_rate"]) == (2, 44100)
    # two distinct stream cfgs for five files, and every file points at its own
    assert len(tb["cfgs"]) == 2 and tb["cfgs"].dtype == pkg.CFG_DTYPE and tb["file_cfg"].dtype == np.uint16
    assert [int(tb["cfgs"][i]["sample_size"]) for i in tb["file_cfg"]] == [16, 24, 16, 16, 24]
    assert len(pkg.corpus_tables([head(pkg, [4096])] * 300)["cfgs"]) == 1
    with pytest.raises(ValueError, match="source 2"):
        pkg.corpus_tables([head(pkg, [1]), head(pkg, [1]), head(pkg, [1], channels=1), head(pkg, [1], rate=48000)])
    with pytest.raises(ValueError, match="source 1"):
        pkg.corpus_tables([head(pkg, [1]), head(pkg, [1], rate=48000)])
    with pytest.raises(ValueError):
        pkg.corpus_tables([])
    # more than 65535 distinct cfgs (the frame length makes them distinct): 0xFFFF stays free for the padding entry
    many = [head(pkg, [1], frame_length=1 + i) for i in range(65536)]
    with pytest.raises(ValueError, match="65535"):
        pkg.corpus_tables(many)
    assert len(pkg.corpus_tables(many[:65535])["cfgs"]) == 65535


def test_the_entry_point_is_declared_bound_and_exported():
    import alac.net_amd as pkg

    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+alacgpu_plan_crops_device\s*\(([^)]*)\)", src)
    assert m, "include/alacgpu.h does not declare alacgpu_plan_crops_device"
    assert len(m.group(1).split(",")) == len(pkg.SYMBOLS["alacgpu_plan_crops_device"][1]) == 21
    assert hasattr(pkg.lib(), "alacgpu_plan_crops_device")
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    assert "alacgpu_plan_crops_device(" in cs
    assert pkg.lib().alacgpu_version() == 3
    # argument checks come before any device work
    assert pkg.lib().alacgpu_plan_crops_device(None, *([None] * 5), 0, None, None, 1, 1, 1, 0, *([None] * 8)) == -1
