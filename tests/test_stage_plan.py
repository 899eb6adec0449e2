"""The host side of a corpus with a host tier: stage_plan_host (the staging kernel's specification), the staging bound S(L)
against every offset of small tables, the split of a corpus's files over the two tiers, and the new entry point's declaration.
CPU only."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def round16(x):
    return (int(x) + 15) // 16 * 16


def test_stage_offsets_are_the_scan_of_the_rounded_counted_sizes():
    import alac.net_amd as pkg

    lo, hi = 1000, 500
    # (offset, size, counts): inside either part, touching both ends of each, size 0, straddling lo, past the end, far away
    cases = [(0, 16, True), (0, 1, True), (5, 15, True), (984, 16, True), (983, 17, True), (983, 18, False), (999, 2, False),
             (1000, 17, True), (1000, 500, True), (1000, 501, False), (1483, 17, True), (1484, 17, False), (1500, 0, True),
             (1500, 1, False), (1501, 0, False), (7, 0, True), (2 ** 64 - 1, 1, False), (2 ** 64 - 1, 2 ** 32 - 1, False),
             (0, 2 ** 32 - 1, False), (0, 1000, True), (0, 1001, False), (17, 16400 % 900, True), (17, 17, True), (17, 17, True)]
    off = np.array([c[0] for c in cases], dtype=np.uint64)
    size = np.array([c[1] for c in cases], dtype=np.uint32)
    want_counted = [round16(c[1]) if c[2] else 0 for c in cases]
    want_off = np.concatenate([[0], np.cumsum(want_counted)[:-1]])
    total = int(np.sum(want_counted))
    so, t, copied = pkg.stage_plan_host(off, size, lo, hi, 2 ** 40)
    assert so.dtype == np.uint64 and copied.dtype == bool and so.shape == copied.shape == (len(cases),)
    assert so.tolist() == want_off.tolist() and t == total and (so % 16 == 0).all()
    assert copied.tolist() == [w > 0 for w in want_counted]
    # the capacity: exactly at the total, one below (the last counted packet goes, whole), far below; the total does not move
    last = max(j for j, w in enumerate(want_counted) if w)
    for cap in (total, total - 1, total - 16, 100, 16, 15, 0):
        so2, t2, c2 = pkg.stage_plan_host(off, size, lo, hi, cap)
        assert so2.tolist() == want_off.tolist() and t2 == total
        assert c2.tolist() == [w > 0 and int(o) + w <= cap for o, w in zip(want_off, want_counted)]
    assert pkg.stage_plan_host(off, size, lo, hi, total)[2][last] and not pkg.stage_plan_host(off, size, lo, hi, total - 1)[2][last]
    # one part empty: the other is the whole space
    for lo_, hi_ in ((0, 1500), (1500, 0)):
        so3, t3, c3 = pkg.stage_plan_host([0, 1499, 1490, 1500], [16, 1, 11, 0], lo_, hi_, 1000)
        assert so3.tolist() == [0, 16, 32, 32] and t3 == 32 and c3.tolist() == [True, True, False, False]
    so3, t3, c3 = pkg.stage_plan_host([999, 1000], [2, 1], 1000, 0, 100)      # nothing behind lo_bytes
    assert so3.tolist() == [0, 0] and t3 == 0 and not c3.any()
    so3, t3, c3 = pkg.stage_plan_host([0, 0], [0, 1], 0, 0, 100)              # no space at all
    assert t3 == 0 and not c3.any()
    # n = 0
    so0, t0, c0 = pkg.stage_plan_host(np.zeros(0, np.uint64), np.zeros(0, np.uint32), lo, hi, 100)
    assert so0.shape == (0,) and so0.dtype == np.uint64 and t0 == 0 and c0.shape == (0,) and c0.dtype == bool


def brute_force_stage_bytes(pkg, durations, sizes, L):
    """The most staged bytes of a window of L frames over every offset of one file"""
    d = np.asarray(durations, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.int64) if len(d) else np.zeros(0, np.int64)
    T = int(d.sum())
    best = 0
    for o in range(T + 1):
        p0, p1 = pkg.window_plan(first, d, o, min(L, T - o))[:2]
        best = max(best, sum(round16(s) for s in sizes[p0:max(p1, p0)]))
    return best


def test_stage_bytes_per_crop_is_the_exact_maximum():
    import alac.net_amd as pkg
    from test_corpus_plan import TABLES, tables_of

    rng = np.random.default_rng(33)
    small = [[min(int(x), 40) for x in t] for t in TABLES]      # (every offset is tried: the long durations cut down)
    trials = [TABLES, small] + [[rng.integers(0, 8, int(rng.integers(0, 40))).tolist() for _ in range(int(rng.integers(1, 5)))]
                                for _ in range(40)]
    for k, files in enumerate(trials):
        tb = tables_of(files, rng)
        lengths = (1, 17, 4097, 20000) if k == 0 else (1, 2, 3, 5, 8, 13, 40, 1000)
        for L in lengths:
            S = pkg.stage_bytes_per_crop(tb["pkt_size"], tb["pkt_end"], tb["file_first"], L)
            best = 0
            for f, d in enumerate(files):
                g0, g1 = int(tb["file_first"][f]), int(tb["file_first"][f + 1])
                best = max(best, brute_force_stage_bytes(pkg, d, tb["pkt_size"][g0:g1].tolist(), L))
            assert best == S, (k, L)           # no offset of any file stages more, and one stages as much
            # ... and through the plan: the staged bytes of the plan of a crop are those of its packets
            K = max(pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L), 1)
            crops = [(f, o) for f, d in enumerate(trials[k]) for o in rng.integers(0, int(np.sum(d)) + 1, 6)]
            cf, co = np.array([c[0] for c in crops], np.uint32), np.array([c[1] for c in crops], np.uint64)
            plan = pkg.corpus_plan_host(tb["pkt_offset"], tb["pkt_size"], tb["pkt_end"], tb["file_first"], tb["file_cfg"], cf, co, L, K, 2 * L)
            total_bytes = int(tb["pkt_size"].sum())
            so, total, copied = pkg.stage_plan_host(plan[0], plan[1], total_bytes // 2, total_bytes - total_bytes // 2, len(crops) * S)
            per_crop = np.add.reduceat(np.where(plan[1] > 0, (plan[1].astype(np.int64) + 15) // 16 * 16, 0), np.arange(0, len(crops) * K, K))
            assert (per_crop <= S).all() and total <= len(crops) * S, (k, L)
        assert pkg.stage_bytes_per_crop(tb["pkt_size"], tb["pkt_end"], tb["file_first"], 0) == 0
    # one frame length: never above K(L) packets of the largest size
    tb = tables_of([[4096] * 40])
    for L in (1, 4096, 4097, 88200):
        K = pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L)
        assert pkg.stage_bytes_per_crop(tb["pkt_size"], tb["pkt_end"], tb["file_first"], L) <= K * round16(tb["pkt_size"].max())
    assert pkg.stage_bytes_per_crop(np.zeros(0, np.uint32), np.zeros(0, np.uint64), [0, 0], 5) == 0


def test_the_tier_split_takes_the_longest_prefix_that_fits():
    import alac.net_amd as pkg

    sizes = [100, 50, 0, 200, 10]
    run = np.cumsum(sizes).tolist()                # 100 150 150 350 360
    assert pkg.tier_split(sizes, None) == 5
    assert pkg.tier_split(sizes, 0) == 0           # everything on the host
    assert pkg.tier_split(sizes, 99) == 0          # one byte short of the first file: it is not split
    assert pkg.tier_split(sizes, 100) == 1         # an exact fit
    assert pkg.tier_split(sizes, 149) == 1
    assert pkg.tier_split(sizes, 150) == 3         # (a file without bytes goes along)
    assert pkg.tier_split(sizes, 349) == 3 and pkg.tier_split(sizes, 350) == 4 and pkg.tier_split(sizes, 359) == 4
    assert pkg.tier_split(sizes, 360) == 5 and pkg.tier_split(sizes, 10 ** 15) == 5 and pkg.tier_split(sizes, np.int64(360)) == 5
    for h in range(0, 400, 7):                     # the prefix rule: files 0 .. k fit, file k does not
        k = pkg.tier_split(sizes, h)
        assert (k == 0 or run[k - 1] <= h) and (k == len(sizes) or run[k] > h)
    # a small file behind one that did not fit stays on the host: a prefix, not a knapsack
    assert pkg.tier_split([100, 1000, 1], 150) == 1
    assert pkg.tier_split([], 5) == 0 and pkg.tier_split([0, 0], 0) == 2
    for bad in (-1, 1.5, "3", True, np.float32(2)):
        with pytest.raises(ValueError):
            pkg.tier_split(sizes, bad)


def test_the_staging_entry_point_is_declared_bound_and_exported():
    import alac.net_amd as pkg

    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+alacgpu_stage_packets_device\s*\(([^)]*)\)", src)
    assert m, "include/alacgpu.h does not declare alacgpu_stage_packets_device"
    assert len(m.group(1).split(",")) == len(pkg.SYMBOLS["alacgpu_stage_packets_device"][1]) == 13
    assert hasattr(pkg.lib(), "alacgpu_stage_packets_device")
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    assert "alacgpu_stage_packets_device(" in cs
    # argument checks come before any device work
    assert pkg.lib().alacgpu_stage_packets_device(None, None, 0, None, 0, None, None, 1, None, 0, None, None, None) == -1
    # the constructor's own check needs no device either
    for bad in (-1, 2.5, "1"):
        with pytest.raises(ValueError):
            pkg.Corpus([], hbm_bytes=bad)
