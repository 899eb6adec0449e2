"""The host side of a corpus whose files differ in sample rate: corpus_tables(mixed_rates=True), corpus_plan_host with a
window length per crop against the scalar form crop by crop, the K and S bounds with a window length per file against every
offset of small tables, the tables of a call with a table per row, and the two entry points' declarations.  CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as tests/test_corpus_plan.py has them: regular with a short last packet, one packet, zero-duration packets, irregular, a
# duration above the longest frame, no frames, no packets
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


def tables_of(duration_lists, rng):
    counts = [len(d) for d in duration_lists]
    file_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    pkt_end = np.concatenate([np.cumsum(np.asarray(d, dtype=np.int64)) for d in duration_lists] + [np.zeros(0, np.int64)])
    pkt_size = rng.integers(0, 5000, int(file_first[-1])).astype(np.uint32)
    pkt_offset = np.concatenate([[0], np.cumsum(pkt_size.astype(np.uint64))[:-1]]).astype(np.uint64)[:len(pkt_size)]
    file_cfg = (np.arange(len(duration_lists)) % 3).astype(np.uint16)
    return dict(pkt_offset=pkt_offset, pkt_size=pkt_size, pkt_end=pkt_end.astype(np.uint64), file_first=file_first, file_cfg=file_cfg)


def head(pkg, durations, sample_size=16, channels=2, rate=44100):
    return dict(sizes=np.full(len(durations), 100, np.uint32), durations=np.asarray(durations, dtype=np.int64),
                cfg=pkg.make_cfgs([(4096, sample_size, 40, 10, 14, channels)]), num_channels=channels, sample_rate=rate)


def test_corpus_tables_take_files_of_different_rates_when_asked():
    import alac.net_amd as pkg

    heads = [head(pkg, [4096, 4096, 10], rate=44100), head(pkg, [4096, 7], 24, rate=48000), head(pkg, [1024] * 5, rate=16000)]
    tb = pkg.corpus_tables(heads, mixed_rates=True)
    assert tb["file_rate"].tolist() == [44100, 48000, 16000] and tb["file_rate"].dtype == np.int64
    assert tb["sample_rate"] is None and tb["channels"] == 2
    # everything else: the three single-file corpora, one behind the other
    singles = [pkg.corpus_tables([h]) for h in heads]
    assert tb["num_frames"].tolist() == [int(s["num_frames"][0]) for s in singles]
    assert np.array_equal(tb["pkt_end"], np.concatenate([s["pkt_end"] for s in singles]))
    assert np.array_equal(tb["pkt_size"], np.concatenate([s["pkt_size"] for s in singles]))
    assert np.array_equal(np.diff(tb["file_first"].astype(np.int64)), [len(s["pkt_size"]) for s in singles])
    assert np.array_equal(np.diff(tb["file_base"].astype(np.int64)), [s["blob_bytes"] for s in singles])
    assert tb["blob_bytes"] == sum(s["blob_bytes"] for s in singles)
    for f, s in enumerate(singles):
        g = int(tb["file_first"][f])
        assert np.array_equal(tb["pkt_offset"][g:g + len(s["pkt_offset"])], s["pkt_offset"] + tb["file_base"][f])
        assert tb["cfgs"][int(tb["file_cfg"][f])] == s["cfgs"][0]
    # one rate: the corpus of the default, with the rates listed
    same = [head(pkg, [4096, 3]), head(pkg, [17], 24)]
    a, b = pkg.corpus_tables(same), pkg.corpus_tables(same, mixed_rates=True)
    assert a["sample_rate"] == b["sample_rate"] == 44100 and b["file_rate"].tolist() == [44100, 44100]
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    # the default refuses as it always did; the channel count is checked either way
    with pytest.raises(ValueError, match=r"source 1: 2 channels at 48000 Hz, the first has 2 at 44100 Hz"):
        pkg.corpus_tables(heads)
    with pytest.raises(ValueError, match=r"source 1: 2 channels at 48000 Hz, the first has 2 at 44100 Hz"):
        pkg.corpus_tables(heads, mixed_rates=False)
    with pytest.raises(ValueError, match="source 2: 1 channels"):
        pkg.corpus_tables(heads[:2] + [head(pkg, [5], channels=1, rate=44100)], mixed_rates=True)
    for mixed in (False, True):
        with pytest.raises(ValueError, match="source 1: 1 channels"):
            pkg.corpus_tables([heads[0], head(pkg, [5], channels=1, rate=44100)], mixed_rates=mixed)


def test_plan_with_a_length_per_crop_is_the_scalar_plan_crop_by_crop():
    import alac.net_amd as pkg

    rng = np.random.default_rng(33)
    tb = tables_of(TABLES, rng)
    tabs = (tb["pkt_offset"], tb["pkt_size"], tb["pkt_end"], tb["file_first"], tb["file_cfg"])
    totals = [int(np.sum(d)) for d in TABLES]
    bound, stride = 9000, 2 * 9000
    crops = [(f, int(o)) for f in range(len(TABLES)) for o in sorted({0, totals[f] // 2, totals[f]} | set(rng.integers(0, totals[f] + 1, 4).tolist()))]
    crops += [(len(TABLES), 0), (0, totals[0] + 1), (2 ** 32 - 1, 5)]
    each = rng.integers(0, bound + 1, len(crops)).astype(np.uint32)
    each[:4] = (0, 1, bound, bound)
    over = [5, 11]                      # lengths above the bound: no such crop
    each[over] = (bound + 1, 2 ** 32 - 1)
    cf, co = np.array([c[0] for c in crops], dtype=np.uint32), np.array([c[1] for c in crops], dtype=np.uint64)
    for K in (1, 3, 12):
        got = pkg.corpus_plan_host(*tabs, cf, co, bound, K, stride, crop_frames=each)
        assert [a.dtype for a in got] == [np.uint64, np.uint32, np.uint16, np.uint64, np.uint32, np.uint32, np.int64]
        for b in range(len(crops)):
            one = pkg.corpus_plan_host(*tabs, cf[b:b + 1], co[b:b + 1], int(each[b]), K, stride)
            j = slice(b * K, (b + 1) * K)
            if b in over:
                assert got[6][b] == -1 and (got[2][j] == 0xFFFF).all() and not any(got[i][j].any() for i in (0, 1, 3, 4, 5))
                continue
            assert got[6][b] == one[6][0], (b, K)
            for i in (0, 1, 2, 4, 5):
                assert np.array_equal(got[i][j], one[i]), (b, K, i)
            used = one[2] != 0xFFFF     # a single crop is row 0: the rows differ by b * stride in the entries that are packets
            assert np.array_equal(got[3][j], np.where(used, one[3] + np.uint64(b * stride), 0)), (b, K)
        assert (got[6][-3:] == -1).all() and (got[6] == -2).any() == (K < 12)
    # the default and a constant array: today's plan
    a = pkg.corpus_plan_host(*tabs, cf, co, 5000, 4, 10000)
    for kw in (dict(crop_frames=None), dict(crop_frames=np.full(len(crops), 5000, np.uint32))):
        b_ = pkg.corpus_plan_host(*tabs, cf, co, 5000, 4, 10000, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(a, b_))
    with pytest.raises(ValueError):
        pkg.corpus_plan_host(*tabs, cf, co, 5000, 4, 10000, crop_frames=[1, 2])


def brute_force(durations, sizes, L):
    """(the most packets, the most staged bytes) of a window of L frames over every offset of one file"""
    import alac.net_amd as pkg

    d = np.asarray(durations, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.int64) if len(d) else np.zeros(0, np.int64)
    rounded = (np.asarray(sizes, dtype=np.int64) + 15) // 16 * 16
    T = int(d.sum())
    k = s = 0
    for o in range(T + 1):
        p0, p1 = pkg.window_plan(first, d, o, min(L, T - o))[:2]
        k, s = max(k, p1 - p0), max(s, int(rounded[p0:p1].sum()))
    return k, s


def test_k_and_s_with_a_length_per_file_are_the_exact_maxima():
    import alac.net_amd as pkg

    rng = np.random.default_rng(44)
    for trial in range(50):
        # durations that vary, zeros among them, and short last packets
        files = [rng.integers(0, 8, int(rng.integers(0, 40))).tolist() + [int(rng.integers(0, 3))] for _ in range(int(rng.integers(1, 5)))]
        if trial % 5 == 0:
            files.append([])
        tb = tables_of(files, rng)
        for lens in ([int(x) for x in rng.choice([0, 1, 2, 3, 5, 8, 13, 40, 1000], len(files))] for _ in range(4)):
            want = [brute_force(d, tb["pkt_size"][int(tb["file_first"][f]):int(tb["file_first"][f + 1])], L) if L > 0 else (0, 0)
                    for f, (d, L) in enumerate(zip(files, lens))]
            assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], np.array(lens)) == max(w[0] for w in want), (files, lens)
            assert pkg.stage_bytes_per_crop(tb["pkt_size"], tb["pkt_end"], tb["file_first"], lens) == max(w[1] for w in want), (files, lens)
        # a constant array is the scalar
        for L in (0, 1, 5, 40):
            const = np.full(len(files), L, dtype=np.int64)
            assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], const) == pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L)
            assert pkg.stage_bytes_per_crop(tb["pkt_size"], tb["pkt_end"], tb["file_first"], const) == \
                pkg.stage_bytes_per_crop(tb["pkt_size"], tb["pkt_end"], tb["file_first"], L)
    # a short window in the file of many packets, a long one in the file of few: each file is bounded by its own length
    tb = tables_of([[10] * 50, [10] * 50], rng)
    assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], [11, 101]) == 11
    assert pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], [11, 0]) == 2
    with pytest.raises(ValueError):
        pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], [11, 101, 5])


def test_the_tables_of_a_call_with_a_table_per_row():
    from alac.net_amd.resample import identity_table, resample_table, rows_tables

    table_of, desc, d0, w = rows_tables([44100, 48000, 16000, 44100, 22050, 48000], 16000)
    assert table_of.tolist() == [0, 1, 2, 0, 3, 1] and desc.dtype == np.uint32 and desc.shape == (4, 5)
    assert d0.dtype == np.int32 and w.dtype == np.float32
    for t, want in enumerate((resample_table(44100, 16000), resample_table(48000, 16000), identity_table(), resample_table(22050, 16000))):
        a, b, width, d0_first, w_first = (int(x) for x in desc[t])
        assert (a, b, width) == want[:3]
        assert np.array_equal(d0[d0_first:d0_first + b], want[3]) and np.array_equal(w[w_first:w_first + b * (2 * width + 1)], want[4].reshape(-1))
    assert len(d0) == int(desc[:, 1].sum()) and len(w) == int((desc[:, 1] * (2 * desc[:, 2] + 1)).sum())
    with pytest.raises(ValueError, match=r"source 2: .*16384"):
        rows_tables([44099, 88198, 44100, 48000], 44099)
    with pytest.raises(ValueError):
        rows_tables([44100, 0], 16000)


def test_the_entry_points_are_declared_bound_and_refuse_null():
    import alac.net_amd as pkg

    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    for name, n_args in (("alacgpu_plan_crops_frames_device", 22), ("alacgpu_resample_rows_device", 18)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"include/alacgpu.h does not declare {name}"
        assert len(m.group(1).split(",")) == len(pkg.SYMBOLS[name][1]) == n_args
        assert hasattr(pkg.lib(), name) and name + "(" in cs
    assert pkg.lib().alacgpu_version() == 3
    # argument checks come before any device work
    assert pkg.lib().alacgpu_plan_crops_frames_device(None, *([None] * 5), 0, None, None, None, 1, 1, 1, 0, *([None] * 8)) == -1
    assert pkg.lib().alacgpu_resample_rows_device(None, None, 1, 1, 0, None, None, None, 1, None, None, 1, None, None, None, 0, None, None) == -1
