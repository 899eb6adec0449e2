"""alac_level_measure_kernel and alac_level_apply_kernel by code path, as tests/test_features_paths.py does it for the log-mel
kernel: a named grid GRID of (rate, channels, T, lengths, modes), each case there for one branch of csrc/alac_level.hip that
tests/test_level.py (hops of 800, 1103 and 1600 frames, at most 7 blocks, two channels, 8209 frames) does not reach --

    a hop longer than a tile, carried through open_hop[] over two and three tiles (48000 and 44100 Hz), a hop that is a tile
    (40960 Hz: every he == t0 + TILE) and one that divides it (5120 Hz: no chunk straddles, second[] is all zero);
    more than ALAC_LEVEL_BATCH blocks (3200 Hz, 259, 260 and 300 hops), with blocks below either gate in both batches;
    three, four and five channels, the surround channels loud enough that their weight decides which blocks pass the gate;
    rows above ALAC_LEVEL_PART * ALAC_LEVEL_MAX_PARTS frames: parts of 8192 frames, their seam, their tail and their early return;
    raw hops of 16, 17, 4095, 4097 and 9000 frames through the C ABI, which the public call's rates do not give.

The host tests need no device: the grid is what it says (plain arithmetic on the constants of level.py and biquad.py), the
signals reach both gates where they are meant to, and the twin is within the module's bound of the sequential specification
`level_host` on every new shape.  The GPU tests hold the kernel to the twin bit for bit -- the output, g, E and P --, the
sentinels behind v and in the rows that are not written, and the output to U32 |s| + U32 peak of `level_host`.  Every T of
the grid is odd, so a contiguous tensor has an odd stride and both launches go scalar; the cases that name the "aligned" layout
(a slice of planes whose stride is a multiple of four floats) run the 16-byte loads of the measure launch and the 16-byte
loads and stores of the apply launch -- for the long rows up to the seam of two parts and with a part's tail behind them --,
and the host test asserts which layout takes which.

Which case takes which route to the specification.  `level_host` is a Python loop over the samples, so it is computed (once,
shared by the host and the GPU tests) for the cases of at most 35 000 frames a plane: every "hop-" case and the three
"channels-" cases; there the kernel is held to `level_host` directly.  The cases "blocks-" (96 007 frames) and "long-row-"
(1 052 673 frames) go by way of the twin: `test_the_twin_is_the_specification_on_shortened_rows` holds the twin to `level_host`
on rows of the same construction cut short, and the GPU test holds the kernel to the twin.  The raw hops are held to
`_measure` and `_gain` of level.py, the functions the twin is made of."""
import functools
import os
import re
import sys

import numpy as np
import pytest

from test_level_spec import ROOT, U32, specs

gpu = pytest.mark.gpu
SENT = 1234.5
SURROUND = 1.41                    # BS.1770's weight of Ls and Rs
EBU_CASE_6 = (-28.0, -28.0, -24.0, -30.0, -30.0)         # dBFS of L, R, C, Ls, Rs; EBU Tech 3341 reads -23.0 +- 0.1 LUFS


def mod():
    import alac.net_amd  # noqa: F401

    return sys.modules["alac.net_amd.level"]


def consts():
    from alac.net_amd.biquad import CHUNK, TILE
    from alac.net_amd.level import BATCH, MAX_PARTS, PART

    return TILE, CHUNK, BATCH, PART, MAX_PARTS


def part_frames(frames):
    """alac_level_part_frames of alac_level.h"""
    TILE, CHUNK, BATCH, PART, MAX_PARTS = consts()
    least = (frames + PART - 1) // PART
    k = (least + MAX_PARTS - 1) // MAX_PARTS
    return PART * max(k, 1)


LONG = 4096 * 256 + 4097           # PART * MAX_PARTS + 4097 (the host test holds the constants to it)


def laid_out(lay, T):
    """(the stride of a plane, the floats the base is off 16 bytes) of x [B, C, T] in a layout of tests/test_level.py's `layouts`"""
    return {"contiguous": (T, 0), "aligned": ((T + 7) // 4 * 4, 0), "odd": (T + 1 + T % 2, 0), "odd-base": (T, 1)}[lay]


def takes_16_bytes(lay, T):
    """Whether the entry sets vec and vec_out, the 16-byte loads and stores of both launches (alacgpu_level_device: the base and
    the stride are multiples of 16 bytes; the tests' outputs have their source's layout)"""
    stride, off = laid_out(lay, T)
    return off == 0 and stride % 4 == 0


def hop_lengths(hop, T):
    """Around four hops (the least a loudness needs), six hops, a last whole hop that ends inside a tile with frames behind it
    in the same tile (5 hop + 100), and everything"""
    return (4 * hop - 1, 4 * hop, 6 * hop, 6 * hop + 17, 5 * hop + 100, T)


# name: (rate, channels, T, lengths, modes, layouts).  A "hop-" and a "channels-" case is held to level_host, the others to the twin.
GRID = {
    "hop-over-three-tiles-48000": (48000, 2, 7 * 4800 + 123, hop_lengths(4800, 7 * 4800 + 123), ("lufs", "peak", "rms-clamp"), ("contiguous", "aligned", "odd-base")),
    "hop-straddles-chunk-and-tile-44100": (44100, 2, 7 * 4410 + 123, hop_lengths(4410, 7 * 4410 + 123), ("lufs",), ("contiguous", "aligned")),
    "hop-is-a-tile-40960": (40960, 1, 6 * 4096 + 77, (4 * 4096 - 1, 4 * 4096, 5 * 4096 + 1, 6 * 4096, 6 * 4096 + 77), ("lufs",), ("contiguous",)),
    "hop-divides-a-tile-5120": (5120, 2, 19 * 512 + 5, (4 * 512 - 1, 4 * 512, 8 * 512, 16 * 512, 16 * 512 + 1, 19 * 512 + 5),
                                ("lufs", "lufs-max-peak", "rms-clamp"), ("contiguous",)),
    "blocks-260-hops-3200": (3200, 2, 300 * 320 + 7, (259 * 320 + 5, 260 * 320, 300 * 320 + 7, 300 * 320 + 7), ("lufs", "lufs-max-peak"), ("contiguous", "aligned")),
    "channels-3-8000": (8000, 3, 8209, (8209, 8192, 4100), ("lufs", "rms"), ("contiguous",)),
    "channels-4-8000": (8000, 4, 8209, (8209, 8192, 4100), ("lufs", "rms"), ("contiguous",)),
    "channels-5-8000": (8000, 5, 8209, (8209, 8192, 4100), ("lufs", "rms"), ("contiguous",)),
    "long-row-1-channel": (48000, 1, LONG, (LONG - 4097, LONG - 4096, LONG, 5000), ("peak", "rms-clamp"), ("contiguous", "aligned", "odd-base")),
    "long-row-2-channels": (48000, 2, LONG, (LONG - 4097, LONG - 4096, LONG, 5000), ("peak", "rms-clamp"), ("contiguous", "aligned", "odd-base")),
    "long-row-lufs-48000": (48000, 1, LONG, (LONG,), ("lufs",), ("contiguous", "aligned")),
}
# the stretches of the 260-hop rows, in hops: (first, behind the last, the factor or the amplitude); "abs": noise at 1e-5
BLOCK_ROWS = ([(100, 140, "rel")], [(100, 140, "rel"), (250, 260, "rel")], [(100, 140, "rel"), (270, 290, "rel")], [(60, 80, "abs"), (262, 282, "abs")])
# ... and of the same rows cut short for the specification: 19, 20 and 40 hops, the stretches where the long rows have them
SHORT_BLOCK_LENGTHS = (19 * 320 + 5, 20 * 320, 40 * 320 + 7, 40 * 320 + 7)
SHORT_BLOCK_ROWS = ([(6, 11, "rel")], [(6, 11, "rel"), (15, 20, "rel")], [(6, 11, "rel"), (30, 36, "rel")], [(6, 12, "abs"), (26, 34, "abs")])
RAW_HOPS = (16, 17, 4095, 4097, 9000)


def stretched(seed, C, T, hop, plans):
    """Rows of noise at 0.2, every row with its stretches of whole hops 40 dB down ("rel") or at 1e-5 ("abs")"""
    rng = np.random.default_rng(seed)
    x = 0.2 * rng.standard_normal((len(plans), C, T))
    for b, plan in enumerate(plans):
        for h0, h1, kind in plan:
            if kind == "rel":
                x[b, :, h0 * hop:h1 * hop] *= 0.01
            else:
                x[b, :, h0 * hop:h1 * hop] = 1e-5 * rng.standard_normal((C, (h1 - h0) * hop))
    return x.astype(np.float32)


def surround_rows(C, T, hop):
    """Three rows at 1, 1/2 and 1/4 of: the front channels at 0.05 and the surround channels at 0.2 over the first five hops,
    behind them the surround channels nearly silent and the front ones at the level that puts a block of them between the two
    relative gates -- the one with the surround weight 1.41 and the one with 1.0.  With seven blocks of which two are all
    front, the mean of the blocks is about (e_loud + e_late) / 2, so a late block passes where e_late > e_loud / 19."""
    rng = np.random.default_rng(C)
    x = rng.standard_normal((3, C, T))
    F, S, ns = 0.05 ** 2, 0.2 ** 2, max(C - 3, 0)
    loud = lambda w: 3 * F + w * ns * S
    late = loud(1.0) / 19.0 * np.sqrt(loud(SURROUND) / loud(1.0))           # midway, in decibels, between the two gates
    amp = np.empty((C, T))
    amp[:3, :5 * hop], amp[3:, :5 * hop] = 0.05, 0.2
    amp[:3, 5 * hop:], amp[3:, 5 * hop:] = np.sqrt(late / 3.0), 1e-4
    return (np.array([1.0, 0.5, 0.25])[:, None, None] * amp * x).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows(name):
    """(x float32 [B, C, T], lengths) of a case, a row per length: noise as in test_level_spec.rows; read-only.  A row of a
    "hop-" case with six whole hops or more has everything from 50 frames in front of its last block on 40 dB down, so that
    the relative gate rejects that block."""
    rate, C, T, lengths, modes, lays = GRID[name]
    assert not name.startswith("long-row-")                    # (long_rows)
    hop = mod().hop_frames(rate)
    B = len(lengths)
    if name.startswith("blocks-"):
        x = stretched(rate, C, T, hop, BLOCK_ROWS)
    elif name.startswith("channels-"):
        x = surround_rows(C, T, hop)
    else:
        rng = np.random.default_rng(rate)
        amp = np.array([0.3, 0.2, 0.05, 0.5, 0.1, 0.25, 0.125])[:B]
        x = amp[:, None, None] * rng.standard_normal((B, C, T))
        for b, v in enumerate(lengths):
            if v // hop >= 6:
                x[b, :, (v // hop - 4) * hop - 50:] *= 0.01
        x = x.astype(np.float32)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x, np.array(lengths)


@functools.lru_cache(maxsize=None)
def long_noise():
    """[2, 1, LONG] of noise at 0.25 and 0.1"""
    rng = np.random.default_rng(LONG)
    return (np.array([0.25, 0.1])[:, None, None] * rng.standard_normal((2, 1, LONG))).astype(np.float32)


def long_rows(name):
    """The long rows two at a time, so that no tensor is above 8.5 MB: [(x, lengths)]"""
    rate, C, T, lengths, modes, lays = GRID[name]
    if C == 1:
        x = long_noise()
        return [(x[:len(lengths[i:i + 2])], np.array(lengths[i:i + 2])) for i in range(0, len(lengths), 2)]
    x = long_noise().reshape(1, 2, LONG)
    return [(x, np.array([v])) for v in lengths]


@functools.lru_cache(maxsize=None)
def twin_of(name, mode, part=0):
    """(y, g, E, P) of level_host_twin on a case (on the part-th tensor of a long-row case), computed once"""
    import alac.net_amd as pkg

    rate = GRID[name][0]
    x, lens = long_rows(name)[part] if name.startswith("long-row-") else rows(name)
    return pkg.level_host_twin(x, specs()[mode], rate, lens, details=True)


@functools.lru_cache(maxsize=None)
def spec_of(name, mode):
    """(s, g, E, P) of level_host on a "hop-" or "channels-" case, computed once"""
    import alac.net_amd as pkg

    assert name.startswith(("hop-", "channels-")) and GRID[name][2] <= 35000
    x, lens = rows(name)
    return pkg.level_host(x, specs()[mode], GRID[name][0], lens, details=True)


def block_energies(x, v, hop, q, weights):
    """e[j] of one row x [C, T] from the twin's hop sums, with the given channel weights"""
    lv = mod()
    s = lv._measure(x[None], np.array([v]), hop, q, True)[2][0]
    nb = s.shape[1] - 3
    z = ((s[:, 0:nb] + s[:, 1:nb + 1]) + (s[:, 2:nb + 2] + s[:, 3:nb + 3])) / np.float64(4 * hop)
    e = np.float64(weights[0]) * z[0]
    for c in range(1, s.shape[0]):
        e = e + np.float64(weights[c]) * z[c]
    return e


def gates(e):
    """(above the absolute gate, above both) of block energies"""
    lv = mod()
    above = e > lv.GATE_ABS
    return above, above & (e > lv.GATE_REL * e[above].mean())


def within_the_bound(y, s):
    err = np.abs(np.asarray(y, dtype=np.float64) - s)
    peak = np.abs(s).max(axis=(1, 2), keepdims=True)
    return bool(np.all(err <= U32 * np.abs(s) + U32 * peak)), float((err / np.maximum(peak, 1e-300)).max())


# ---- without a device ------------------------------------------------------------------------------------------------------------
def whole_hops_over(hop, v, tiles):
    """The whole hops k of a row of v frames that have frames in `tiles` tiles or more"""
    TILE = consts()[0]
    return [k for k in range(v // hop) if (k * hop + hop - 1) // TILE - k * hop // TILE + 1 >= tiles]


def test_the_grid_is_what_it_says():
    lv = mod()
    TILE, CHUNK, BATCH, PART, MAX_PARTS = consts()
    assert (TILE, CHUNK, BATCH, PART, MAX_PARTS) == (4096, 16, 256, 4096, 256) and LONG == PART * MAX_PARTS + 4097
    hops = {name: lv.hop_frames(GRID[name][0]) for name in GRID}
    for name, (rate, C, T, lengths, modes, lays) in GRID.items():
        assert max(lengths) == T and all(m in specs() for m in modes) and lays[0] == "contiguous", name
        assert T <= 35000 or not name.startswith(("hop-", "channels-")), name          # what level_host is computed for

    # a hop over three tiles: a whole hop k and a tile t0 with k hop < t0 and (k + 1) hop > t0 + TILE -- the middle tile
    # reads open_hop[] and writes it
    name = "hop-over-three-tiles-48000"
    hop, (rate, C, T, lengths, modes, lays) = hops[name], GRID[name]
    assert hop == 4800 > TILE and [takes_16_bytes(lay, T) for lay in lays] == [False, True, False] and lays[2] == "odd-base"
    middle = lambda v: [(k, t0) for k in range(v // hop) for t0 in range(0, v, TILE) if k * hop < t0 and (k + 1) * hop > t0 + TILE]
    assert middle(T) == [(5, 6 * TILE)] and whole_hops_over(hop, T, 3) == [5]
    assert [bool(middle(v)) for v in lengths] == [False, False, True, True, False, True]
    assert set(lengths) >= {4 * hop - 1, 4 * hop, 6 * hop, 6 * hop + 17, T}
    # ... and a length whose last whole hop ends inside a tile with frames behind it in that tile
    assert any(v % hop and (v // hop * hop) % TILE and (v // hop * hop) // TILE == (v - 1) // TILE for v in lengths)
    # every hop of it crosses a tile boundary: open_hop[] is read in every tile but the first
    assert all(k * hop // TILE != ((k + 1) * hop - 1) // TILE for k in range(T // hop))

    # 44100 Hz: a hop that is no multiple of a chunk, so a chunk straddles the boundary of hops that also cross tiles
    name = "hop-straddles-chunk-and-tile-44100"
    hop, (rate, C, T, lengths, modes, lays) = hops[name], GRID[name]
    assert hop == 4410 > TILE and hop % CHUNK != 0 and lengths == hop_lengths(hop, T)      # (the same lengths in hops)
    assert [takes_16_bytes(lay, T) for lay in lays] == [False, True]
    for k in range(1, T // hop):
        assert (k * hop) % CHUNK != 0 and (k * hop) // TILE != ((k + 1) * hop - 1) // TILE, k

    # a hop that is a tile: every he == t0 + TILE, s[] is written from every tile and open_hop[] never
    name = "hop-is-a-tile-40960"
    hop, T = hops[name], GRID[name][2]
    assert hop == TILE and T // hop >= 6 and T % hop and whole_hops_over(hop, T, 2) == []

    # a hop that divides a tile: hop boundaries on chunk and tile boundaries, no chunk straddles (second[] is all zero)
    name = "hop-divides-a-tile-5120"
    hop, (rate, C, T, lengths, modes, lays) = hops[name], GRID[name]
    assert hop == 512 and TILE % hop == 0 and hop % CHUNK == 0 and T > 2 * TILE and 2 * TILE in lengths and 2 * TILE + 1 in lengths
    assert whole_hops_over(hop, T, 2) == []

    # more than a batch of blocks: exactly one batch, one block into the second, well into it
    name = "blocks-260-hops-3200"
    hop, lengths = hops[name], GRID[name][3]
    assert hop == 320 and [v // hop for v in lengths] == [259, 260, 300, 300]
    assert [v // hop - 3 for v in lengths[:3]] == [BATCH, BATCH + 1, BATCH + 41] and len(BLOCK_ROWS) == len(lengths)
    assert [v // hop for v in SHORT_BLOCK_LENGTHS] == [19, 20, 40, 40]
    assert [takes_16_bytes(lay, GRID[name][2]) for lay in GRID[name][5]] == [False, True]

    # three, four and five channels, a little over two tiles
    for C in (3, 4, 5):
        rate, ch, T, lengths, modes, lays = GRID[f"channels-{C}-8000"]
        assert ch == C and 2 * TILE < T < 2 * TILE + CHUNK * 2 and "lufs" in modes and C <= lv.MAX_CHANNELS

    # a row over 256 parts: parts of two PART, a seam that is not where a row of PART-frame parts has one, and a tail
    assert part_frames(LONG) == 2 * PART == 8192 and part_frames(PART * MAX_PARTS) == PART and part_frames(PART * MAX_PARTS + 1) == 2 * PART
    src = open(os.path.join(ROOT, "alac.net_amd", "csrc", "alac_level.h")).read()
    body = re.search(r"alac_level_part_frames\(uint64_t frames\)\s*\{(.*?)\n\}", src, re.S).group(1)
    for line in ("least = (frames + ALAC_LEVEL_PART - 1u) / ALAC_LEVEL_PART;", "k = (least + ALAC_LEVEL_MAX_PARTS - 1u) / ALAC_LEVEL_MAX_PARTS;",
                 "return (uint64_t)ALAC_LEVEL_PART * (k ? k : 1u);"):
        assert line in body, line
    for C in (1, 2):
        rate, ch, T, lengths, modes, lays = GRID[f"long-row-{C}-channel" + "s" * (C - 1)]
        assert ch == C and T == LONG and set(lengths) == {PART * MAX_PARTS, PART * MAX_PARTS + 1, LONG, 5000}
        assert set(modes) == {"peak", "rms-clamp"}
        # LONG is odd, so a contiguous tensor of it has an odd stride and is scalar in both launches, as the odd base is; only
        # the aligned layout (a stride of LONG + 3 floats) takes the 16-byte loads and stores.  There every part begins on 16
        # bytes, the float4 loop runs up to the seam of two parts of 8192 frames, and the last part is 4096 frames of 16-byte
        # stores and a tail of one; a row of PART * MAX_PARTS + 1 frames has a last part that is a tail alone
        assert [(lay, takes_16_bytes(lay, LONG)) for lay in lays] == [("contiguous", False), ("aligned", True), ("odd-base", False)]
        assert laid_out("aligned", LONG)[0] % 4 == 0 and part_frames(LONG) % 4 == 0 and LONG % part_frames(LONG) == 4097
        assert (PART * MAX_PARTS + 1) % part_frames(LONG) == 1
        # a row of 5000 frames has frames in one part of 129
        assert -(-5000 // part_frames(LONG)) == 1 and -(-LONG // part_frames(LONG)) == 129
    assert GRID["long-row-lufs-48000"][:4] == (48000, 1, LONG, (LONG,))
    assert [takes_16_bytes(lay, LONG) for lay in GRID["long-row-lufs-48000"][5]] == [False, True]

    # the raw hops: one hop per lane of the hop loop and more than a batch of blocks; either side of a tile; over four tiles
    assert RAW_HOPS[0] == lv.MIN_HOP == CHUNK and TILE // 16 == lv.THREADS and raw_frames(16) // 16 - 3 > BATCH and raw_frames(16) <= 4300
    assert 17 % CHUNK and (4095, 4097) == (TILE - 1, TILE + 1)
    assert whole_hops_over(9000, raw_frames(9000), 4) == [5] and all(raw_frames(h) // h >= 6 for h in RAW_HOPS)
    assert all(takes_16_bytes("aligned", raw_frames(h)) and not takes_16_bytes("odd", raw_frames(h)) for h in RAW_HOPS)


def test_the_signals_reach_the_gates():
    lv = mod()
    BATCH = consts()[2]
    # the 260-hop rows: blocks rejected by either gate in the first batch and in the second
    name = "blocks-260-hops-3200"
    x, lens = rows(name)
    q, hop = lv.kweight(3200), 320
    rejected = []
    for b in range(len(lens)):
        above, both = gates(block_energies(x[b], int(lens[b]), hop, q, lv.WEIGHTS))
        j = np.arange(len(above))
        rejected.append([int((~above & (j < BATCH)).sum()), int((~above & (j >= BATCH)).sum()),
                         int((above & ~both & (j < BATCH)).sum()), int((above & ~both & (j >= BATCH)).sum())])
    print("blocks below the absolute gate (first batch, second), below the relative one alone (first, second):", rejected)
    assert rejected[0][2] >= 1 and rejected[0][1] == rejected[0][3] == 0          # (256 blocks: no second batch)
    assert rejected[1][2] >= 1 and rejected[1][3] == 1                            # block 256, the only one of its batch
    assert rejected[2][2] >= 1 and rejected[2][3] >= 1
    assert rejected[3][0] >= 1 and rejected[3][1] >= 1
    # the hop rows of six hops or more: the relative gate rejects the last block
    for name in GRID:
        if name.startswith("hop-"):
            x, lens = rows(name)
            rate = GRID[name][0]
            hop = lv.hop_frames(rate)
            for b in np.nonzero(lens // hop >= 6)[0]:
                above, both = gates(block_energies(x[b], int(lens[b]), hop, lv.kweight(rate), lv.WEIGHTS))
                assert above.all() and not both[-1] and both[0], (name, b)
    # the surround channels: their weight decides which blocks pass
    for C in (3, 4, 5):
        x, lens = rows(f"channels-{C}-8000")
        for b in (0, 1):
            real = gates(block_energies(x[b], int(lens[b]), 800, lv.kweight(8000), (1.0, 1.0, 1.0, SURROUND, SURROUND)))[1]
            ones = gates(block_energies(x[b], int(lens[b]), 800, lv.kweight(8000), (1.0,) * 5))[1]
            print(f"{C} channels, row {b}: blocks that pass with the surround weight {real.astype(int)}, with 1.0 {ones.astype(int)}")
            assert (C == 3) == np.array_equal(real, ones), C
            assert real[0] and (C == 3 or (ones[-1] and not real[-1]))


@pytest.mark.parametrize("name", [n for n in GRID if n.startswith(("hop-", "channels-"))])
def test_the_twin_is_within_the_bound_of_the_specification(name):
    rate, C, T, lengths, modes, lays = GRID[name]
    hop = mod().hop_frames(rate)
    for mode in modes:
        (s, g, E, P), (y, gt, Et, Pt) = spec_of(name, mode), twin_of(name, mode)
        rel = np.abs(gt / g - 1.0)
        ok, worst = within_the_bound(y, s)
        print(f"{name} {mode}: max |g_twin / g_host - 1| = {rel.max():.3e}, the twin's output at most {worst:.3e} of the row's peak off")
        assert np.array_equal(P, Pt) and np.all(rel <= U32) and np.array_equal(g == 1.0, gt == 1.0) and ok
        if mode.startswith("lufs"):
            assert np.array_equal(g != 1.0, np.array(lengths) >= 4 * hop)


def test_the_twin_is_the_specification_on_shortened_rows():
    """The route of the "blocks-" and "long-row-" cases: rows of the same construction, short enough for level_host"""
    import alac.net_amd as pkg

    lv = mod()
    TILE, CHUNK, BATCH, PART, MAX_PARTS = consts()
    x = stretched(3200, 2, SHORT_BLOCK_LENGTHS[-1], 320, SHORT_BLOCK_ROWS)
    lens = np.array(SHORT_BLOCK_LENGTHS)
    for b in range(4):
        above, both = gates(block_energies(x[b], int(lens[b]), 320, lv.kweight(3200), lv.WEIGHTS))
        assert (not above.all()) == (b == 3) and not both.all(), b
    cases = [(x, lens, 3200, ("lufs", "lufs-max-peak"))]
    n = 2 * PART + 4097
    for C in (1, 2):
        short = long_noise()[..., :n] if C == 1 else long_noise()[..., :n].reshape(1, 2, n).repeat(2, axis=0)
        cases += [(np.ascontiguousarray(short), np.array(v), 48000, ("peak", "rms-clamp")) for v in ((2 * PART, 2 * PART + 1), (n, 5000))]
    n = 5 * 4800 + 4097
    cases.append((np.ascontiguousarray(long_noise()[:1, :, :n]), np.array([n]), 48000, ("lufs",)))
    for x, lens, rate, modes in cases:
        for mode in modes:
            s, g, E, P = pkg.level_host(x, specs()[mode], rate, lens, details=True)
            y, gt, Et, Pt = pkg.level_host_twin(x, specs()[mode], rate, lens, details=True)
            rel = np.abs(gt / g - 1.0)
            ok, worst = within_the_bound(y, s)
            print(f"{x.shape} at {rate} Hz {mode}: max |g_twin / g_host - 1| = {rel.max():.3e}, output {worst:.3e} of the peak")
            assert np.array_equal(P, Pt) and np.all(rel <= U32) and (g != 1.0).all() and ok


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch

    import alac.net_amd as pkg

    return torch, pkg, sys.modules["alac.net_amd.level"]


def on_device(torch, x, lay):
    """x [B, C, T] on the device in one layout of tests/test_level.py's `layouts`, built the same way: contiguous, the slice
    [..., :T] of wider planes of sentinels, or a base 4 bytes off 16"""
    B, C, n = x.shape
    stride, off = laid_out(lay, n)
    if stride == n:
        flat = torch.full((B * C * n + 4,), SENT, device="cuda")
        d = flat[off:off + B * C * n].view(B, C, n)
    else:
        d = torch.full((B, C, stride), SENT, device="cuda")[..., :n]
    d.copy_(torch.from_numpy(np.array(x)))
    assert d.stride(1) == stride and d.data_ptr() % 16 == 4 * off
    return d


def held_to_the_twin(env, x, lens, spec, rate, ref, lays, tag):
    """The entry into sentinels, the public call and the call in place on every layout of `lays` against ref = (y, g, E, P) of
    the twin, bit for bit; returns the public call's output of the first layout as numpy"""
    from test_level import measured, same

    torch, pkg, lv = env
    twin, gt, Et, Pt = ref
    T = x.shape[2]
    v = np.clip(lens, 0, T)
    written = (gt != 1.0) | (spec.clamp & (Et != 0.0) & (v > 0))
    first = None
    for lay in lays:
        d = on_device(torch, x, lay)
        out = torch.empty_strided(d.shape, d.stride(), dtype=d.dtype, device="cuda").fill_(SENT)
        got_g, got_E, got_P = measured(torch, pkg, lv, d, spec, rate, lens, out)
        got = out.cpu().numpy()
        assert same(got_g, gt) and same(got_E, Et) and same(got_P, Pt), (tag, lay, got_g, gt, got_E, Et)
        for b in range(len(lens)):
            if written[b]:
                assert same(got[b, :, :v[b]], twin[b, :, :v[b]]), (tag, lay, b)
                assert (got[b, :, v[b]:] == SENT).all(), (tag, lay, b)
            else:
                assert (got[b] == SENT).all(), (tag, lay, b)
        y = pkg.level(d, spec, rate, lens)
        assert same(y.cpu().numpy(), twin), (tag, lay)
        first = y if first is None else first
        assert torch.equal(y.view(torch.int32), first.view(torch.int32)), (tag, lay)
        assert pkg.level(d, spec, rate, lens, out=d) is d and torch.equal(d.view(torch.int32), first.view(torch.int32)), (tag, lay)
        if d._base is not None and d._base.dim() == 3:
            assert bool((d._base[..., T:] == SENT).all()), (tag, lay)          # behind the slice nothing was written
    return first.cpu().numpy()


@gpu
@pytest.mark.parametrize("name", [n for n in GRID if not n.startswith("long-row-")])
def test_the_kernel_is_its_twin_on_the_grid(env, name):
    """The "hop-" and "channels-" cases also within the bound of level_host; "blocks-" by way of the twin (the module docstring)"""
    rate, C, T, lengths, modes, lays = GRID[name]
    x, lens = rows(name)
    for mode in modes:
        got = held_to_the_twin(env, x, lens, specs()[mode], rate, twin_of(name, mode), lays, (name, mode))
        if name.startswith(("hop-", "channels-")):
            ok, worst = within_the_bound(got, spec_of(name, mode)[0])
            print(f"{name} {mode}: kernel against the specification at most {worst:.3e} of the row's peak")
            assert ok, (name, mode)


@gpu
@pytest.mark.parametrize("name", [n for n in GRID if n.startswith("long-row-")])
def test_the_kernel_is_its_twin_on_long_rows(env, name):
    """By way of the twin (the module docstring); in place against out of place inside held_to_the_twin"""
    rate, C, T, lengths, modes, lays = GRID[name]
    for part, (x, lens) in enumerate(long_rows(name)):
        for mode in modes:
            held_to_the_twin(env, x, lens, specs()[mode], rate, twin_of(name, mode, part), lays, (name, mode, part))


@gpu
def test_measure_only_gives_the_same_numbers(env):
    """d_out null, so parts == 1: g, E and P of the three-tile case are the bits they are with an output, with scalar and with
    16-byte loads"""
    from test_level import measured, same

    torch, pkg, lv = env
    name = "hop-over-three-tiles-48000"
    x, lens = rows(name)
    for lay in ("contiguous", "aligned"):
        d = on_device(torch, x, lay)
        for mode in ("lufs", "rms-clamp", "peak"):
            spec = specs()[mode]
            alone = measured(torch, pkg, lv, d, spec, 48000, lens, None)
            twin, gt, Et, Pt = twin_of(name, mode)
            assert same(alone[0], gt) and same(alone[1], Et) and same(alone[2], Pt), (lay, mode)
            assert np.array_equal(d.cpu().numpy().view(np.int32), x.view(np.int32))


def raw_frames(hop):
    """Six whole hops and 77 frames; for 16 a little over a tile, more than a batch of blocks"""
    return 4200 if hop == 16 else 6 * hop + 77


def raw_twin(lv, x, lens, hop, q, spec):
    """level_host_twin with a hop that no rate gives: _measure and _gain of level.py, then fl32(g x)"""
    B, C, T = x.shape
    v = np.clip(lens, 0, T)
    P, S, s = lv._measure(x, v, hop, q, True)
    y, g, E = x.copy(), np.ones(B), np.zeros(B)
    for b in range(B):
        g[b], E[b], measured = lv._gain(spec, C, int(v[b]), hop, P[b], S[b], s[b] if s[b] is not None else np.zeros((C, 0)))
        if measured and (g[b] != 1.0 or spec.clamp):
            r = (g[b] * x[b, :, :v[b]].astype(np.float64)).astype(np.float32)
            y[b, :, :v[b]] = np.minimum(np.maximum(r, np.float32(-1)), np.float32(1)) if spec.clamp else r
    return y, g, E, P


@gpu
@pytest.mark.parametrize("hop", RAW_HOPS)
def test_raw_hops_through_the_c_abi(env, hop):
    from alac.net_amd.resample import _context
    from test_level import same

    torch, pkg, lv = env
    T = raw_frames(hop)
    rng = np.random.default_rng(hop)
    lens = np.array([T, 4 * hop, 4 * hop - 1, 5 * hop + 3])
    x = np.array([0.3, 0.1, 0.2, 0.05])[:, None, None] * rng.standard_normal((4, 2, T))
    x[0, :, (T // hop - 4) * hop - 5:] *= 0.01                  # the relative gate rejects the last block
    x = x.astype(np.float32)
    q = lv.kweight(8000)
    d_q = torch.from_numpy(q).cuda()
    valid = torch.from_numpy(lens).cuda()
    for spec in (lv.Level.lufs(-23.0), lv.Level.lufs(-10.0, max_peak=0.9, clamp=True)):
        twin, gt, Et, Pt = raw_twin(lv, x, lens, hop, q, spec)
        assert list(gt != 1.0) == [True, True, False, True]
        for lay in ("aligned", "odd"):                           # 16-byte and scalar loads and stores
            d = on_device(torch, x, lay)
            out = torch.empty_strided(d.shape, d.stride(), dtype=d.dtype, device="cuda").fill_(SENT)
            res = [torch.full((4,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
            _context(0).level_device(d, out, 4, 2, d.stride(1), T, valid, lv.LUFS, hop, d_q, spec.linear, spec.max_peak or 0.0, spec.clamp,
                                     *res, stream=torch.cuda.current_stream().cuda_stream)
            got, (got_g, got_E, got_P) = out.cpu().numpy(), [r.cpu().numpy() for r in res]
            assert same(got_g, gt) and same(got_E, Et) and same(got_P, Pt), (hop, lay, got_g, gt, got_E, Et)
            for b in range(4):
                if gt[b] != 1.0:
                    assert same(got[b, :, :lens[b]], twin[b, :, :lens[b]]) and (got[b, :, lens[b]:] == SENT).all(), (hop, lay, b)
                else:
                    assert (got[b] == SENT).all(), (hop, lay, b)
            assert bool((d._base[..., T:] == SENT).all()), (hop, lay)


def ebu_case_6(seconds, rate=48000):
    """EBU Tech 3341 case 6: 997 Hz in L, R, C, Ls, Rs (the channel order of alac_level.h), float32 [1, 5, seconds rate]"""
    t = np.arange(int(seconds * rate)) / rate
    return np.stack([(10.0 ** (db / 20.0) * np.sin(2.0 * np.pi * 997.0 * t)).astype(np.float32) for db in EBU_CASE_6])[None]


@gpu
def test_ebu_case_6_on_the_gpu(env):
    from test_level import measured, same

    torch, pkg, lv = env
    x = ebu_case_6(2)
    d = torch.from_numpy(x).cuda()
    got = float(pkg.loudness(d, 48000)[0])
    y, gt, Et, Pt = pkg.level_host_twin(x, lv.Level.lufs(), 48000, details=True)
    print("EBU Tech 3341 case 6 on the GPU:", got)
    assert abs(got - -23.0) <= 0.1 and abs(got - (-0.691 + 10.0 * np.log10(Et[0]))) <= 1e-12
    g, E, P = measured(torch, pkg, lv, d, lv.Level.lufs(), 48000, None, None)
    assert same(g, gt) and same(E, Et) and same(P, Pt)
