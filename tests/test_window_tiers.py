"""The window builds (the *_win kernels behind alacgpu_decode_window_into_device, what Corpus.crops runs) on the directed packets of
tests/tier_cases.py: the store-pattern cases -- zero runs against the unit and chunk grid (f), runs up to and past the packet's
end (f_ends), eight rates and a packet that ends early in one workgroup (l), the highest bit rates (k_59, k_34) -- and two FIR
groups, with windows that begin at DIRECTED frames: 0, 1, either side of the unit grid (8, 16) and of the chunk grid (32), the
packet's last frame, the first frame behind it and one further.  The output wave packs end << 16 | skip into one register and
decides each store from two sign bits of one subtraction (alac_kernels.hip: store_sample), alac_dst_fill_kernel zero-fills from
max(n - skip, 0): an off-by-one in either shows as a sample where a canary or a zero belongs, or the other way round.

The harness is tests/test_decode_window.py's: canaries outside every run, the oracle's frames inside, zeros behind the decoded
frames; statuses and sample counts equal to alacgpu_decode_into_device's on the same batch.  Where a window begins -- inside a
zero run that lasts to the packet's end or beyond it, on the first frame behind a packet that ends early, inside an escape-coded
stretch -- is asserted from the writer's trace before anything runs."""
import numpy as np
import pytest

import tier_cases as tc
from test_decode_window import Dev, arrangement, check, expected, pkg, reference, run, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FORMS = [("int32", "interleaved"), ("float32", "planar")]       # (the other two: tests/test_decode_window.py, on encoder packets)
ROUNDS = 2                                                      # per form: 4 x 16 windows per batch
N_SKIPS, N_COUNTS = 14, 4


def skip_choices(n):
    return [min(max(s, 0), 16384) for s in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, n - 1, n, n + 1)]


def directed_windows(n_dec, rnd):
    """Window of the packet at batch position i in round rnd: the skips cycle through skip_choices, the frame counts through
    `exactly to the end`, 1, `40 past the end` and 0; the runs lie one behind the other with canary gaps of 0..4 frames."""
    # (A batch position meets four of the fourteen skips, one per round; all fourteen are met over the sixteen positions of
    # every round.  Which skip falls on which packet is index arithmetic: the pairings the cases are there for -- a start
    # inside the silent packet's run, on the frame behind an early end -- are pinned by assert_window_premises, not by this.)
    count = len(n_dec)
    skip = np.array([skip_choices(int(n_dec[i]))[(i + 5 * rnd) % N_SKIPS] for i in range(count)], dtype=np.int64)
    room = np.maximum(n_dec - skip, 0)
    kind = (np.arange(count) // 2 + np.arange(count) + rnd) % N_COUNTS
    frames = np.choose(kind, [room, np.ones(count, np.int64), room + 40, np.zeros(count, np.int64)])
    gaps = (np.arange(count) * 3 + rnd) % 5
    first = np.cumsum(gaps) + np.concatenate([[0], np.cumsum(frames)[:-1]])
    return first, frames, skip, int(first[-1] + frames[-1]) + 3


def all_rounds(n_dec):
    return [directed_windows(n_dec, rnd) for rnd in range(ROUNDS * len(FORMS))]


def starts(g, b, rounds):
    """(packet, its first channel's trace, skip, frames) of every window of every round"""
    return [(j, g.traces[j][0], int(skip[i]), int(frames[i])) for _, frames, skip, _ in rounds for i, j in enumerate(b["order"])]


def assert_window_premises(name, g, b, rounds):
    w = starts(g, b, rounds)
    if name == "l":
        # Strictly inside a zero run that lasts to the packet's last frame.  (No run of case l passes the end: its longest, the
        # silent packet's, is run(n - 1) behind one value.  A start inside a run that does pass the end is f_ends', below.)
        # On the unit or chunk grid, one off it, and on the run's -- and the packet's -- last frame:
        in_run = {s for j, tr, s, f in w for t in tr if t.kind == "r" and t.index + 1 < s <= t.index + t.value == g.ns[j] - 1 and f > 0}
        n_silent = max(g.ns)
        assert in_run & {8, 16, 32} and in_run & {7, 9, 15, 17, 31, 33} and n_silent - 1 in in_run, sorted(in_run)
        # ... and on the first frame behind the packet that is shorter than its neighbours
        assert any(g.ns[j] < max(g.ns) and s == g.ns[j] and f > 0 for j, tr, s, f in w)
    if name == "f_ends":
        # strictly inside a zero run that continues past the packet's end, in a packet the reference decodes
        assert any(t.kind == "r" and t.index + 1 < s <= t.index + t.value and t.index + t.value > g.ns[j] - 1 and s < g.ns[j] and f > 0
                   and g.status[j] == 0 for j, tr, s, f in w for t in tr), "no window begins inside a run past the end"
        # on the first frame behind the end of a packet that ends early (640 of the stream's 4096 frames)
        assert any(g.ns[j] < g.cfgs[g.cfg_idx[j]][0] and s == g.ns[j] and f > 0 and tr[-1].kind == "r" and g.status[j] == 0
                   for j, tr, s, f in w), "no window begins behind an early end"
    if name.startswith("k_"):
        # inside an escape-coded stretch: the symbol of the window's first frame and its neighbours are escape codes
        def escaped(tr, s):
            at = [t for t in tr if t.kind == "v" and s - 1 <= t.index <= s + 1]
            return len(at) == 3 and all(t.escape for t in at)
        assert any(0 < s < g.ns[j] - 1 and f > 0 and escaped(tr, s) for j, tr, s, f in w), "no window begins among escape codes"


def check_group(torch, pkg, oracle, g, key, name=""):
    b = g.batch()
    channels = int(g.cfgs[0][5])
    ref = reference(oracle, key, b)
    assert ref[3].tolist() == b["status"] and ref[2].tolist() == [g.ns[j] for j in b["order"]]
    n_dec = np.clip(ref[2].astype(np.int64), 0, 16384)
    rounds = all_rounds(n_dec)
    assert_window_premises(name, g, b, rounds)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        for k, (first, frames, skip, total) in enumerate(rounds):
            dtype, layout = FORMS[k % len(FORMS)]
            out, os_, st = run(torch, ctx, d, first, frames, skip, dtype, layout, channels, total)
            _, os_old, st_old = run(torch, ctx, d, first, frames, None, dtype, layout, channels, total, window=False)
            assert np.array_equal(st, st_old) and np.array_equal(st, ref[3]), (k, dtype, layout, st, st_old)
            assert np.array_equal(os_, os_old) and np.array_equal(os_, ref[2]), (k, dtype, layout)
            check(out, expected(b, ref, first, frames, skip, st, dtype, layout, channels, total),
                  f"{g.name} round {k} {dtype} {layout} (packets {b['order']}, skips {skip.tolist()}, frames {frames.tolist()})")


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("name", ["k_59", "k_34", "f", "f_ends", "l"])
def test_store_pattern_cases_through_the_window_builds(torch, pkg, oracle, name, stereo, is24):
    g = tc.build(name, stereo, is24, tc.ORDER_CLASSES[(stereo + 2 * is24) % 3])
    check_group(torch, pkg, oracle, g, ("tiers", name, stereo, is24), name)


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("kind", ["uniform", "warmup"])
def test_fir_groups_through_the_window_builds(torch, pkg, oracle, kind, stereo, is24):
    # full-range residuals over every order 1..16 and beyond (both launches), and packets of one to three frames
    check_group(torch, pkg, oracle, tc.build_fir(kind, stereo, is24, 0), ("tiers_fir", kind, stereo, is24))
