"""Directed packets for the entropy tiers and the FIR waves, built with rice_writer (tests only).

Every case is a workgroup of eight packets whose Rice streams are written symbol by symbol.  A builder first asserts the case's
premise from the writer's trace -- a statement about the bitstream, for unit sizes 8 and 16 both -- and returns the packets;
tests/test_rice_writer.py runs every builder on the CPU (premises, both oracles), tests/test_entropy_tiers.py compares the GPU with
the oracle on them; tests/test_fir_steps.py does so per build of the FIR step (FIR groups of one order class, Group.embed for the
four-tap step), tests/test_window_tiers.py through the window builds.  Sample i of a channel belongs to unit i // U and chunk i // 32.
"""
import functools
import random
import zlib

import numpy as np

import rice_writer as rw
from rice_writer import ChannelWriter

VARIANTS = [(False, False), (True, False), (False, True), (True, True)]      # (stereo, is24): rss 16, 17, 24, 25
ORDER_CLASSES = ["first_launch", "two_taps", "second_launch"]              # orders 1..8, 9..16, {0, 17..30, 31}
UNITS = (8, 16)
# The second launch gives orders above 16 two FIR waves (16 lanes per stream, two taps per lane) in launches of up to this many
# groups of eight packets, and the one wave with four taps per lane above it: ALAC_L16_MAX_GROUPS of alac_kernels.hip, which
# tests/test_rice_writer.py reads back, so that a retuned threshold cannot move the embedded batches off the four-tap step
L16_MAX_GROUPS = 256
EMBED_GROUPS = L16_MAX_GROUPS + 1                  # Group.embed: 8 * 256 + 8 == 2056 packets in one launch
EMBED_PACKETS = 8 * EMBED_GROUPS
PLAIN = 3000            # a history level without run symbols or escape codes (k = 3)


def _orders(oc, j, c, n):
    if oc == "first_launch":
        return 1 + (3 * j + c) % 8
    if oc == "two_taps":
        return 9 + (3 * j + c) % 8
    o = [0, 17, 31, 24, 30, 0, 20, 31][(j + c) % 8]
    return 23 if o == 0 and n > 4096 else o       # order 0 above 4096 samples: the reference throws


def _header(oc, j, c, n, ricemod):
    order = _orders(oc, j, c, n)
    r = random.Random(1000 * j + c)
    return rw.channel_header(order=order, coefs=[r.randrange(-200, 200) for _ in range(order)], quant=9, ricemod=ricemod)


def finish(cw, level=PLAIN):
    while not cw.done:
        if cw.expects_run:
            cw.run(0)
        else:
            cw.hold(level, 1)


class Group:
    """eight packets: cfgs (stream configurations), cfg_idx / packets / traces / status per packet"""

    def __init__(self, name, cfgs, cfg_idx, packets, traces, status, ns):
        self.name, self.cfgs, self.cfg_idx, self.packets, self.traces, self.status, self.ns = name, cfgs, cfg_idx, packets, traces, status, ns

    def batch(self, rolls=(0, 3), slack=64):
        """the group, and the same packets rolled to other positions (16 in a row: one workgroup of the dense arrangement)"""
        order = [(j + r) % len(self.packets) for r in rolls for j in range(len(self.packets))]
        blob, offs = bytearray(), []
        for j in order:
            offs.append(len(blob))
            blob += self.packets[j]
        blob += bytes(slack)
        nc = self.cfgs[0][5]
        return dict(blob=np.frombuffer(bytes(blob), dtype=np.uint8), offsets=np.array(offs, dtype=np.uint64),
                    sizes=np.array([len(self.packets[j]) for j in order], dtype=np.uint32),
                    cfg_idx=np.array([self.cfg_idx[j] for j in order], dtype=np.uint16), stream_cfgs=self.cfgs,
                    slot_ints=max(self.ns) * nc + 8, status=[self.status[j] for j in order], order=order)

    def embed(self, filler, groups=None):
        """the group three times inside a launch of `groups` groups of eight packets (default: one more than the second launch
        gives two FIR waves, so that orders above 16 take the four-taps-per-lane step): at group 0, in the middle (rolled by
        3) and as the last group (rolled by 5); every other group is `filler`'s eight packets -- a warm-up FIR group of at
        most 32 frames per packet.  The same keys as batch(); `order`: the group's own packets as (batch index, packet)."""
        groups = groups or EMBED_GROUPS
        assert groups >= 3 and len(self.packets) == len(filler.packets) == 8 and max(filler.ns) <= 32 and not any(filler.status)
        assert filler.cfgs[0][1] == self.cfgs[0][1] and filler.cfgs[0][5] == self.cfgs[0][5], "filler of another stream layout"
        cfgs = list(self.cfgs)
        if filler.cfgs[0] not in cfgs:
            cfgs.append(filler.cfgs[0])
        fidx = cfgs.index(filler.cfgs[0])
        copies = {0: 0, groups // 2: 3, groups - 1: 5}
        fill_blob = b"".join(filler.packets)
        blob, offs, sizes, ci, status, order = bytearray(), [], [], [], [], []
        for grp in range(groups):
            if grp not in copies:
                pos = len(blob)
                for pkt in filler.packets:
                    offs.append(pos)
                    sizes.append(len(pkt))
                    pos += len(pkt)
                blob += fill_blob
                ci += [fidx] * 8
                status += [0] * 8
                continue
            for j in ((k + copies[grp]) % 8 for k in range(8)):
                order.append((len(offs), j))
                offs.append(len(blob))
                sizes.append(len(self.packets[j]))
                blob += self.packets[j]
                ci.append(self.cfg_idx[j])
                status.append(self.status[j])
        blob += bytes(64)
        nc = self.cfgs[0][5]
        return dict(blob=np.frombuffer(bytes(blob), dtype=np.uint8), offsets=np.array(offs, dtype=np.uint64),
                    sizes=np.array(sizes, dtype=np.uint32), cfg_idx=np.array(ci, dtype=np.uint16), stream_cfgs=cfgs,
                    slot_ints=max(self.ns + filler.ns) * nc + 8, status=status, order=order)


_SYMS = {}          # the steered symbol lists per (case, stereo, is24): what build() below cannot share between order classes


def assemble(name, stereo, is24, oc, n, progs, stream_kw=None, ricemods=None, ns=None, status=None, headers=None, own_b=False):
    """progs[j](cw) drives the writer of packet j's channel A; channel B of a two-channel packet runs progs[(j + 3) % 8]."""
    ss = 24 if is24 else 16
    nc = 2 if stereo else 1
    count = len(progs)
    stream_kw = stream_kw or [{}] * count
    ricemods = ricemods or [4] * count
    ns = ns or [n] * count
    cfgs, cfg_idx = [], []
    for kw in stream_kw:
        cfg = (16384 if max(ns) > 4096 else 4096, ss, kw.get("pb", 40), kw.get("mb", 10), kw.get("kb", 14), nc)
        if cfg not in cfgs:
            cfgs.append(cfg)
        cfg_idx.append(cfgs.index(cfg))
    rss = ss + (1 if stereo else 0)
    syms = _SYMS.get((name, stereo, is24))          # (the symbols do not depend on the LPC orders: steered once)
    if syms is None:
        syms = []
        for j in range(count):
            cw = ChannelWriter(cfgs[cfg_idx[j]], rss, ricemods[j], ns[j])
            progs[j](cw)
            assert cw.done, f"{name}: program {j} stops at sample {cw.index} of {ns[j]}"
            syms.append(cw.symbols)
        _SYMS[(name, stereo, is24)] = syms
    packets, traces, hdrs = [], [], []
    for j in range(count):
        chans = [j, j if own_b else (j + 3) % count][:nc]
        # channel B borrows another packet's program: same cfg, Rice modifier and length, or it runs its own again
        chans = [c if (cfg_idx[c], ricemods[c], ns[c]) == (cfg_idx[j], ricemods[j], ns[j]) else j for c in chans]
        hdr = [headers(j, c) if headers else _header(oc, j, c, ns[j], ricemods[j]) for c in range(nc)]
        pkt, tr, _ = rw.write_packet(cfgs[cfg_idx[j]], ns[j], hdr, [syms[c] for c in chans], mix_shift=2 if stereo else 0,
                                     mix_weight=(j % 3) if stereo else 0)
        packets.append(pkt)
        traces.append(tr)
        hdrs.append(hdr)
    g = Group(name, cfgs, cfg_idx, packets, traces, status or [0] * count, ns)
    g.headers = hdrs
    return g


def plain(level=PLAIN):
    return lambda cw: finish(cw, level)


def _vals(tr):
    return [t for t in tr if t.kind == "v"]


def _runs(tr):
    return [t for t in tr if t.kind == "r"]


def _next_kind(tr, t):
    i = tr.index(t)
    return tr[i + 1].kind if i + 1 < len(tr) else None


# ---- a: history exactly 128 (no run symbol) and exactly 127 (run symbol) at every position of a unit --------------------------------
def case_a(stereo, is24, oc):
    def separate(cw):                       # hist_mult 40: 128 and 127 in separate places
        base = 48
        for p in range(16):
            cw.steer_at(base + p, lambda h: h == 128, 200)
            cw.steer_at(base + 48 + p, lambda h: h == 127, 200)
            cw.run(3)
            base += 96
        finish(cw, 200)

    def consecutive(cw):                    # hist_mult 4: 128, then 127 with the next value (128 - (128 * 4 >> 9) == 127)
        cw.value(0)                         # the history starts at 10: a run symbol at once, and after every run it is 0 again
        for p in range(16):
            cw.run(48 + 33 * p - cw.index)
            cw.value(cw.dv_for_history(128))            # 0 + 32 * 4
            cw.value(cw.dv_for_history(127))
        cw.run(3)
        finish(cw, 140)

    n = 48 + 16 * 96 + 24
    g = assemble("a", stereo, is24, oc, n, [separate, consecutive] + [plain()] * 6, stream_kw=[{}, {"pb": 16}] + [{}] * 6,
                 ricemods=[4, 1] + [4] * 6)
    for j in (0, 1):
        tr = g.traces[j][0]
        at128 = [t for t in _vals(tr) if t.hist == 128]
        at127 = [t for t in _vals(tr) if t.hist == 127]
        assert len(at128) >= 16 and len(at127) >= 16
        assert all(_next_kind(tr, t) == "v" for t in at128) and all(_next_kind(tr, t) == "r" for t in at127)
        assert all(tr[i - 1].hist < 128 for i, t in enumerate(tr) if t.kind == "r")
        for u in UNITS:
            assert {t.index % u for t in at128} == set(range(u)) and {t.index % u for t in at127} == set(range(u))
    tr = g.traces[1][0]
    assert sum(1 for a, b in zip(tr, tr[1:]) if a.hist == 128 and b.kind == "v" and b.hist == 127) == 16
    return g


# ---- b: 0xFFFF and 0x10000 without an escape code (k >= 13), then as escape codes ------------------------------------------------------
def case_b(stereo, is24, oc):
    rss = (24 if is24 else 16) + stereo

    def prog(esc):
        def f(cw):
            # No escape code on the way up (the climb takes values of at most seven ones), and the two streams take turns: the
            # canonical one is done before the other's escape codes begin, so that the unit that meets 0x10000 is a plain one.
            cw.hold(PLAIN, 200 if esc else 4)
            for rep in range(3):
                cw.hold(4_600_000, 22)
                cw.value(0xFFFF, esc)
                cw.hold(4_600_000, 4 + rep)
                if not esc or rss > 16:       # a 16-bit raw field cannot hold 0x10000
                    cw.value(0x10000, esc)
                cw.hold(PLAIN, 7 + rep)
            finish(cw)
        return f

    g = assemble("b", stereo, is24, oc, 360, [prog(False), prog(True)] + [plain()] * 6)
    canon, other = _vals(g.traces[0][0]), _vals(g.traces[1][0])
    assert not any(t.escape for t in canon) and max(t.index for t in canon if t.value >= 0xFFFF) < 190
    assert min(t.index for t in other if t.escape) >= 200
    for j, esc in ((0, False), (1, True)):
        v = _vals(g.traces[j][0])
        a = [t for t in v if t.value == 0xFFFF and t.escape == esc and t.k >= 13]
        b = [t for t in v if t.value == 0x10000 and t.escape == esc and t.k >= 13]
        assert len(a) == 3 and all(t.hist != 0xFFFF and t.hist > 0x10000 for t in a)
        assert len(b) == (3 if not esc or rss > 16 else 0) and all(t.hist == 0xFFFF for t in b)
        assert all(t.x <= 8 for t in a + b) if not esc else all(t.x == 9 for t in a + b)
    return g


# ---- c: k at kmod and kmod - 1; hist_mult 0, 1, 63, 441 ---------------------------------------------------------------------------------
# What is pinned: for every stream, units (of 8 and of 16) whose largest k is exactly rice_kmodifier and units whose largest k is
# rice_kmodifier - 1 -- the history is held just below and just above the lowest history with k == kmod, so the change of k falls
# wherever the hold's dither puts it, not at a chosen position of a unit.  kb 1 has no kmod - 1 half (k is 1 throughout); with kb 17
# k never passes 16 == kmod - 1; with hist_mult 0 the history never moves and k stays 1.  hist_mult 40 (the usual 4 * 10) carries
# the kb sweep; 0, 1, 63 and 441 are the issue's.
C_STREAMS = [  # (kb, pb, ricemod) -> hist_mult = ricemod * (pb // 4)
    (1, 40, 4), (4, 255, 7), (14, 40, 4), (16, 40, 4), (17, 40, 4), (4, 4, 1), (14, 255, 1), (4, 40, 0)]


def case_c(stereo, is24, oc):
    def prog(cw):
        cw.gentle = False
        if cw.hist_mult == 0:                 # the history stays at its initial 10: k == 1, a run symbol after every value
            i = 0
            while not cw.done:
                cw.run(i % 3) if cw.expects_run else cw.value(cw.signmod + i % 5)
                i += 1
            return
        kb = min(cw.kb, 16)
        edge = ((1 << kb) - 3) << 9 if kb >= 2 else PLAIN          # the lowest history with k == kb
        top = 0xFFFF * 512                                          # where a run of 0xFFFF values takes the history
        for rep in range(2):
            cw.hold(max(edge - edge // 16, 200), 60 + rep)
            cw.hold(min(edge + edge // 16, top), 220 if kb >= 16 else 60)
        finish(cw, max(edge - edge // 8, 200))

    g = assemble("c", stereo, is24, oc, 700, [prog] * 8, stream_kw=[dict(kb=kb, pb=pb) for kb, pb, _ in C_STREAMS],
                 ricemods=[rm for _, _, rm in C_STREAMS])
    assert sorted({rm * (pb // 4) for _, pb, rm in C_STREAMS}) == [0, 1, 40, 63, 441]
    for j, (kb, pb, rm) in enumerate(C_STREAMS):
        tr = _vals(g.traces[j][0])
        ks = {t.k for t in tr}
        assert max(ks) <= kb
        if rm == 0:
            assert ks == {1}
            continue
        # per unit: the largest k is kmod in some units and kmod - 1 in others (kb 17: k never passes 16 == kmod - 1)
        for u in UNITS:
            umax = {}
            for t in tr:
                umax[t.index // u] = max(umax.get(t.index // u, 0), t.k)
            if kb <= 16:
                assert kb in umax.values(), (kb, ks)
            if kb >= 2:
                assert kb - 1 in umax.values(), (kb, ks)
    return g


# ---- d: history + 1536 through 2^23 and back, for more and for fewer than 32 units ------------------------------------------------------
def case_d(stereo, is24, oc):
    def prog(cw):
        cw.gentle = False
        cw.hold(PLAIN, 16)
        cw.hold(8_600_000, 16 * 34 + 5)       # > 32 units of 16
        cw.hold(8_000_000, 70)
        cw.hold(8_600_000, 8 * 20 + 3)        # < 32 units of 8
        cw.hold(8_000_000, 40)
        cw.hold(8_600_000, 9)                 # a single unit's worth
        finish(cw, 8_000_000)

    n = 900
    g = assemble("d", stereo, is24, oc, n, [prog, prog] + [plain()] * 6, stream_kw=[{"kb": 16}, {}] + [{}] * 6)
    for j in (0, 1):
        tr = _vals(g.traces[j][0])
        above = [t.hist + 1536 >= 1 << 23 for t in tr]
        cross = [i for i in range(1, n) if above[i] != above[i - 1]]
        assert len(cross) == 6, cross
        spans = [cross[1] - cross[0], cross[3] - cross[2], cross[5] - cross[4]]
        assert spans[0] > 32 * 16 and 8 < spans[1] < 32 * 8 - 16 and spans[2] <= 16, spans
    return g


# ---- e: prefix 7, 8, 9 at each k; (x + 1) << k at 0x10000 and just above with a value <= 0xFFFF ------------------------------------------
def case_e(stereo, is24, oc):
    rss = (24 if is24 else 16) + stereo

    def prog(cw):
        kmax = min(cw.kb, 15)
        for k in range(1, kmax + 1):
            mid = (((3 << k) // 2 - 3) << 9) if k >= 2 else 300
            xs = [7, 8, 9] + {13: [], 14: [3, 4], 15: [1, 2]}.get(k, [])
            for x in xs:
                for _ in range(80):
                    if cw.k() == k:
                        break
                    cw.hold(mid, 1)
                assert cw.k() == k, (k, cw.k(), cw.history)
                dv = cw.dv_with_prefix(x)
                if x == 9:
                    dv = min(dv, (1 << rss) - 1 + cw.signmod)
                    if (dv - cw.signmod) // ((1 << k) - 1) <= 8:
                        continue              # no value of this width has nine ones at this k
                cw.value(dv)
        finish(cw)

    g = assemble("e", stereo, is24, oc, 1500, [prog, prog] + [plain()] * 6, stream_kw=[{}, {"kb": 16}] + [{}] * 6)
    for j, kb in ((0, 14), (1, 16)):
        v = _vals(g.traces[j][0])
        seen = {(t.x, t.k) for t in v}
        kmax = min(kb, 15)
        need = {(x, k) for k in range(1, kmax + 1) for x in (7, 8)} | {(3, 14), (4, 14)}
        need |= {(9, k) for k in range(1, kmax + 1) if 9 * ((1 << k) - 1) < 1 << rss}      # (an escape code: nine ones read)
        need |= {(1, 15), (2, 15)} if kb == 16 else set()
        assert need <= seen, need - seen
        # (x + 1) << k exactly 0x10000, and one step of x above it, with a value that needs no history clamp
        on_edge = {(t.x, t.k) for t in v if t.x <= 8 and (t.x + 1) << t.k == 0x10000 and t.value <= 0xFFFF}
        above = {(t.x, t.k) for t in v if t.x <= 8 and t.x << t.k == 0x10000 and t.value <= 0xFFFF}
        assert on_edge >= {(7, 13), (3, 14)} | ({(1, 15)} if kb == 16 else set()), on_edge
        assert above >= {(8, 13), (4, 14)} | ({(2, 15)} if kb == 16 else set()), above
    return g


# ---- f: zero runs against the unit grid -------------------------------------------------------------------------------------------------
F_LENGTHS = [7, 8, 9, 15, 16, 17, 32, 33]      # U - 1, U, U + 1, 2U, 2U + 1 for U = 8 and 16


def case_f(stereo, is24, oc):
    def prog(length):
        def f(cw):
            base = 48
            for p in range(16):
                cw.steer_at(base + p - 1, lambda h: h < 128, 200)   # the run starts at sample base + p
                cw.run(length)
                base += 96
            finish(cw, 200)
        return f

    g = assemble("f", stereo, is24, oc, 48 + 16 * 96, [prog(ln) for ln in F_LENGTHS])
    for j, ln in enumerate(F_LENGTHS):
        r = _runs(g.traces[j][0])
        assert len(r) == 16 and all(t.value == ln for t in r)
        for u in UNITS:
            assert {(t.index + 1) % u for t in r} == set(range(u))
    return g


def case_f_ends(stereo, is24, oc):
    n = 640

    def to_grid(cw):            # runs that end at a unit's end and at a chunk's end; the pending signModifier crosses with them
        cw.steer_at(99, lambda h: h < 128, 200)
        cw.run(12)              # zeros 100..111
        cw.steer_at(180, lambda h: h < 128, 200)
        cw.run(11)              # zeros 181..191
        finish(cw, 200)

    def at_end(extra):
        def f(cw):
            cw.steer_at(n - 20, lambda h: h < 128, 200)
            cw.run(19 + extra)
        return f

    def silent(cw):
        cw.value(0)
        cw.run(n - 1)

    progs = [to_grid, at_end(0), at_end(1), at_end(1000), at_end(16384), silent, plain(), plain(200)]
    g = assemble("f_ends", stereo, is24, oc, n, progs, status=[0, 0, 0, 0, 5, 0, 0, 0], own_b=True)
    r = _runs(g.traces[0][0])
    assert [(t.index + 1, t.index + t.value) for t in r[:2]] == [(100, 111), (181, 191)]
    assert 111 % 16 == 15 and 111 % 8 == 7 and 191 % 32 == 31
    nxt = [t for t in _vals(g.traces[0][0]) if t.index in (112, 192)]
    assert len(nxt) == 2 and all(t.value >= 1 for t in nxt)           # signModifier pending over the boundary
    ends = [g.traces[j][0][-1] for j in (1, 2, 3, 4)]
    assert [t.kind for t in ends] == ["r"] * 4
    assert [t.index + t.value - (n - 1) for t in ends] == [0, 1, 1000, 16384]
    assert ends[2].index + ends[2].value < 16384 <= ends[3].index + ends[3].value
    assert len(g.traces[5][0]) == 2 and g.traces[5][0][1].value == n - 1
    return g


# ---- g: signModifier over boundaries, runs of length 0, a low history at the last sample ------------------------------------------------
def case_g(stereo, is24, oc):
    n = 320

    def zero_runs(cw):
        for idx in (47, 63, 70, 127, 135, 191):      # ends of units of 16 / 8 / chunks, and mid-unit
            cw.steer_at(idx, lambda h: h < 128, 200)
            cw.run(0, escape=idx == 70)
        cw.steer_at(250, lambda h: h < 128, 200)
        cw.run(5, escape=True)
        finish(cw, 200)

    def low_at_end(cw):
        cw.steer_at(n - 1, lambda h: h < 128, 200)

    g = assemble("g", stereo, is24, oc, n, [zero_runs, low_at_end] + [plain()] * 6)
    tr = g.traces[0][0]
    z = [t for t in _runs(tr) if t.value == 0]
    assert [t.index for t in z] == [47, 63, 70, 127, 135, 191] and [t.escape for t in z] == [False, False, True, False, False, False]
    assert {t.index % 16 for t in z} >= {15, 7} and any(t.index % 32 == 31 for t in z)
    assert all(v.value >= 1 for v in _vals(tr) if v.index - 1 in {t.index for t in z})
    assert [(t.value, t.escape) for t in _runs(tr) if t.value][0] == (5, True)
    last = g.traces[1][0][-1]
    assert last.kind == "v" and last.index == n - 1 and last.hist < 128 and not _runs(g.traces[1][0])
    return g


# ---- h: escape codes d units apart, d = 1..20; a prefix-8 value inside a hold -------------------------------------------------------------
def case_h(stereo, is24, oc):
    def spaced(u):
        at, unit = set(), 4
        at.add(unit * u + 3)
        for d in range(1, 21):
            unit += d
            at.add(unit * u + (3 * d) % u)
        return at

    def prog(esc_at, p8_at=()):
        def f(cw):
            while not cw.done:
                if cw.index in esc_at:
                    cw.value(cw.level_dv(PLAIN), escape=True)
                elif cw.index in p8_at:
                    cw.value(cw.dv_with_prefix(8))
                else:
                    cw.hold(PLAIN, 1)
        return f

    n = 16 * (4 + 210 + 3)
    esc3 = {16 * u + 5 for u in range(10, 200, 30)}
    p8 = {i + 16 * d for i in esc3 for d in (1, 2, 5)}
    g = assemble("h", stereo, is24, oc, n, [prog(spaced(16)), prog(spaced(8)), prog(esc3, p8)] + [plain()] * 5)
    for j, u in ((0, 16), (1, 8)):
        units = [t.index // u for t in _vals(g.traces[j][0]) if t.escape]
        assert [b - a for a, b in zip(units, units[1:])] == list(range(1, 21))
    v = _vals(g.traces[2][0])
    assert {t.index for t in v if t.escape} == esc3 and {t.index for t in v if t.x == 8} == p8, ({t.index for t in v if t.escape} ^ esc3, {t.index for t in v if t.x == 8} ^ p8)
    assert not any(t.escape or t.x >= 8 for j in range(3, 8) for t in _vals(g.traces[j][0]))
    return g


# ---- i: an escape code while a neighbour is mid-run, parked, or reads a new run symbol; the same under sustained escape codes -----------
def case_i(stereo, is24, oc):
    n = 1100
    singles = {165, 330, 492}
    sustained = set(range(600, 1000, 4))

    def escapes(cw):
        while not cw.done:
            cw.value(cw.level_dv(PLAIN), escape=cw.index in singles or cw.index in sustained)

    def runs(cw):
        for idx, ln in ((161, 7), (299, 64), (490, 2), (700, 7), (799, 64), (906, 2)):
            cw.steer_at(idx, lambda h: h < 128, 200)
            cw.run(ln)
        finish(cw, 200)

    g = assemble("i", stereo, is24, oc, n, [escapes, runs] + [plain()] * 6)
    esc = {t.index for t in _vals(g.traces[0][0]) if t.escape}
    assert esc == singles | sustained
    r = [(t.index, t.index + 1, t.index + t.value) for t in _runs(g.traces[1][0])]     # (symbol's sample, first zero, last zero)
    for u in UNITS:
        for (sym, a, b), e, kind in zip(r, (165, 330, 492, 704, 832, 908), ("mid", "parked", "new") * 2):
            lo, hi = e // u * u, e // u * u + u - 1
            if kind == "mid":
                assert a <= e <= b and (a > lo or b < hi) and sym < lo + u      # the run covers part of the escape code's unit
            elif kind == "parked":
                assert a <= lo and hi <= b                                       # ... all of it
            else:
                assert lo <= sym <= hi                                           # the run symbol is read inside it
            assert e in esc
    return g


# ---- j: escape codes at all 32 alignments of the cursor, two back to back ---------------------------------------------------------------
def case_j(stereo, is24, oc):
    def prog(level):
        def f(cw):
            # positions inside the channel's stream; the trace turns them into positions inside the packet below
            cw.value(cw.level_dv(level), escape=True)
            cw.value(cw.level_dv(level), escape=True)
            seen = {0, cw.trace[-1].bitpos & 31}
            while not cw.done:                   # an escape code wherever the cursor stands at an alignment not seen yet
                new = (cw.bitpos & 31) not in seen
                seen.add(cw.bitpos & 31)
                cw.value(cw.level_dv(level) + cw.index * 7 % 11, escape=new)
        return f

    g = assemble("j", stereo, is24, oc, 600, [prog(PLAIN * (j + 1)) for j in range(8)])
    for j in range(8):
        v = _vals(g.traces[j][0])
        assert {t.bitpos & 31 for t in v if t.escape} == set(range(32)), j
        assert v[0].escape and v[1].escape and v[1].bitpos == v[0].bitpos + v[0].bits
    return g


# ---- k: the highest bit rates -----------------------------------------------------------------------------------------------------------
def max_rate(cw):
    """every sample a forced escape code that keeps the history below 128, and a forced escape code for a run of 0"""
    i = 0
    while not cw.done:
        cw.run(0, escape=True) if cw.expects_run else cw.value(cw.signmod + i % 2, escape=True)
        i += 1


def loud_escapes(seed):
    def f(cw):
        r = random.Random(seed)
        top = (1 << cw.rss) - 1
        while not cw.done:
            cw.value(r.randrange(top // 2, top), escape=True)
    return f


def case_k_59(stereo, is24, oc):
    n = 4096 if (stereo and is24) else 1024
    g = assemble("k_59", stereo, is24, oc, n, [max_rate] * 8)
    rss = (24 if is24 else 16) + stereo
    for j in range(8):
        for tr in g.traces[j]:
            bits = sum(t.bits for t in tr)
            assert bits == n * (9 + rss) + (n - 1) * 25 and all(t.escape for t in tr)
            if rss == 25:
                assert bits / n >= 58.9
    return g


def case_k_34(stereo, is24, oc):
    n = 16384 if (stereo and is24) else 2048
    g = assemble("k_34", stereo, is24, oc, n, [loud_escapes(s) for s in range(8)])
    rss = (24 if is24 else 16) + stereo
    for j in range(8):
        for tr in g.traces[j]:
            assert sum(t.bits for t in tr) == n * (9 + rss) and len(tr) == n
            if rss == 25:
                assert sum(t.bits for t in tr) / n >= 34
    return g


# ---- l: eight streams at eight rates -----------------------------------------------------------------------------------------------------
def case_l(stereo, is24, oc):
    n = 2048

    def const(dv):
        def f(cw):
            while not cw.done:
                cw.value(dv)
        return f

    def silent(cw):
        cw.value(0)
        cw.run(cw.n - 1)

    def fast(level):
        def f(cw):
            cw.gentle = False
            finish(cw, level)
        return f

    flat = {"mb": 255}         # with Rice modifier 0 the history stays at 255: k == 1, no run symbols
    progs = [max_rate, loud_escapes(5), fast(8_600_000), plain(30_000), const(1), const(0), silent, plain()]
    g = assemble("l", stereo, is24, oc, n, progs, stream_kw=[{}, {}, {}, {}, flat, flat, {}, {}],
                 ricemods=[4, 4, 4, 4, 0, 0, 4, 4], ns=[n] * 7 + [100])
    rss = (24 if is24 else 16) + stereo
    rate = [sum(t.bits for t in g.traces[j][0]) / g.ns[j] for j in range(8)]
    assert rate[0] >= 33.9 + rss and rate[1] == 9 + rss and 14 <= rate[2] <= 24 and 5 <= rate[3] <= 10, rate
    assert rate[4] == 2 and rate[5] == 1 and rate[6] < 0.05 and g.ns[7] == 100, rate
    return g


# the (case, stereo, is24) whose packets have more than 4096 frames: left out where every packet must fit a 4096-frame stream
# (tests/test_fir_steps.py: the embedded batches); tests/test_rice_writer.py checks the set against the built groups
OVER_4096_FRAMES = {("k_34", True, True)}
CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f, "f_ends": case_f_ends, "g": case_g,
         "h": case_h, "i": case_i, "j": case_j, "k_59": case_k_59, "k_34": case_k_34, "l": case_l}


# ==== FIR ====================================================================================================================================
def fir_replay(res, rss, coefs, q):
    """PredictorDecompressFirAdapt for 1 <= order <= 30 (:284-334), restated for the premises: returns the output, the largest
    coefficient magnitude met, the adaptation steps whose remaining error hit exactly zero with taps still to go (the tie), and
    the steps with a non-zero error over an all-equal history."""
    wrap = lambda v: rw.sign_extend(v, 32)
    order, n = len(coefs), len(res)
    c, out = list(coefs), list(res)
    peak, ties, flat = max(abs(x) for x in c), 0, 0
    for i in range(order):
        if i + 1 < n:
            out[i + 1] = rw.sign_extend(out[i] + out[i + 1], rss)
    for i in range(order + 1, n):
        b = i - order - 1
        s = 0
        for j in range(order):
            s = wrap(s + wrap((out[b + order - j] - out[b]) * c[j]))
        err = out[i]
        out[i] = rw.sign_extend((wrap((1 << q >> 1) + s) >> q) + out[b] + err, rss)
        if err:
            pos = err > 0
            flat += all(out[b + 1 + t] == out[b] for t in range(order))
            p = order - 1
            while p >= 0 and (err > 0 if pos else err < 0):
                val = out[b] - out[b + order - p]
                sg = (val > 0) - (val < 0)
                sg = sg if pos else -sg
                c[p] -= sg
                err -= ((val * sg) >> q) * (order - p)
                peak = max(peak, abs(c[p]))
                p -= 1
                if err == 0 and p >= 0:
                    ties += 1
    return out, peak, ties, flat


FIR_KINDS = ["uniform", "patterns", "drift", "flat_and_tie", "warmup"]


FIR_CLASS_ORDERS = {"first_launch": (1, 8), "two_taps": (1, 16), "second_launch": (17, 30)}
FIR_SPECIAL_KINDS = ("uniform", "patterns", "warmup")      # kinds whose premise asks fir_replay (orders 1..30) nothing


def fir_class_orders(r, order_class):
    """eight orders of one class for a group: (j + 3 c) % 8 of them is stream (packet j, channel c).  Which FIR step a group of
    eight packets runs on follows from its orders alone (alac_kernels.hip: ab_kernel_body): all in 1..8 one tap per lane in the
    first launch, some in 9..16 and none outside 1..16 two taps per lane (second launch; the dense arrangement: first), any
    other order the second launch's four-tap (launches above L16_MAX_GROUPS groups) or 16-lane two-tap step."""
    lo, hi = FIR_CLASS_ORDERS[order_class]
    must = {"first_launch": [1, 8], "two_taps": [16, r.randrange(9, 16), r.randrange(1, 9)], "second_launch": [17, 30]}[order_class]
    orders = must + [r.randrange(lo, hi + 1) for _ in range(8 - len(must))]
    r.shuffle(orders)
    return orders


def fir_group(kind, stereo, is24, block=0, order_class=None):
    """eight packets whose entropy content is plain (canonical codes of the chosen residuals); `block` moves through orders 1..31.
    With an order_class every stream of the group takes its order from that class (fir_class_orders; `block` then only reseeds),
    so that the whole group runs on one build of the FIR step; in the second_launch class of the kinds in FIR_SPECIAL_KINDS
    channel A of packet 2 has order 31 and the last channel of packet 5 order 0 (the modes of the special step)."""
    ss = 24 if is24 else 16
    nc = 2 if stereo else 1
    rss = ss + stereo
    cfg = (4096, ss, 40, 10, 14, nc)
    top = (1 << (rss - 1)) - 1
    key = (kind, stereo, is24, block) if order_class is None else (kind, stereo, is24, block, order_class)
    r = random.Random(zlib.crc32(repr(key).encode()))
    class_orders = fir_class_orders(r, order_class) if order_class else None
    packets, traces, ns, facts = [], [], [], dict(peak=0, ties=0, flat=0, lo=0, hi=0, orders=[])
    for j in range(8):
        n = 160
        hdrs, syms = [], []
        for c in range(nc):
            order = 1 + (8 * block + j + 15 * c) % 31
            special = False
            if order_class:
                order = class_orders[(j + 3 * c) % 8]
                if order_class == "second_launch" and kind in FIR_SPECIAL_KINDS and (j, c) in ((2, 0), (5, nc - 1)):
                    order, special = (31 if j == 2 else 0), True
            q = [0, 1, 9, 15][(j + c + block) % 4]
            coefs = [r.choice([r.randrange(-32768, 32768), r.randrange(-3000, 3000)]) for _ in range(order)]
            if kind == "uniform":
                res = [r.randrange(-top - 1, top + 1) for _ in range(n)]
            elif kind == "patterns":
                m = [1, 1, 1, top, top, top, 0, 1][j]
                pat = ["pos", "neg", "alt", "pos", "neg", "alt", "pos", "rnd"][j]
                res = [{"pos": m, "neg": -m, "alt": m if i % 2 else -m, "rnd": r.choice([-1, 0, 1])}[pat] for i in range(n)]
            elif kind == "drift":
                if not order_class:
                    order = [1, 2, 4, 8, 12, 16, 24, 30][(j + c) % 8]
                q = [15, 9, 1, 0][(j + block) % 4]
                coefs = [32767 if (j + t) % 2 == 0 else -32768 for t in range(order)]
                res = [(1 if j % 2 else -1) * (1 + (i % 3 == 0)) for i in range(n)]
            elif kind == "flat_and_tie":
                if not order_class:
                    order = [1, 2, 3, 4, 6, 8, 12, 20][(j + c) % 8]
                q = [0, 0, 1, 2][(j + block) % 4]
                coefs = [r.randrange(-3, 4) << q for _ in range(order)]
                # a constant output (all-equal history), a first error against it, then small errors over small differences
                res = [5] + [0] * (order + 3) + [r.choice([-3, -2, -1, 1, 2, 3, 4, 6]) for _ in range(n - order - 4)]
            else:   # warmup: n from 1 to order + 2
                if not order_class:
                    order = [1, 4, 8, 12, 20, 30][block % 6]
                    n = 1 + (8 * (block // 6) + j) % (order + 2)
                elif c == 0:      # (the packet's length goes by channel A's order; orders 0 and 31 have no warm-up: a few samples)
                    n = 1 + (8 * block + 5 * j) % (order + 2 if order < 31 else 9)
                q = 9
                coefs = [r.randrange(-3000, 3000) for _ in range(order)]
                res = [r.randrange(-top - 1, top + 1) for _ in range(n)]
            if kind != "warmup" and 1 <= order <= 30:
                _, peak, ties, flat = fir_replay(res, rss, coefs, q)
                facts["peak"] = max(facts["peak"], peak)
                facts["ties"] += ties
                facts["flat"] += flat
            facts["lo"], facts["hi"] = min(facts["lo"], min(res)), max(facts["hi"], max(res))
            facts["orders"].append((order, special))
            hdrs.append(rw.channel_header(order=order, coefs=coefs, quant=q, ricemod=4))
            syms.append(rw.symbols_for_residuals(cfg, rss, 4, res))
        pkt, tr, _ = rw.write_packet(cfg, n, hdrs, syms, mix_shift=2 if stereo else 0, mix_weight=(j % 3) if stereo else 0)
        packets.append(pkt)
        traces.append(tr)
        ns.append(n)
    g = Group(f"fir_{kind}" + (f"_{order_class}" if order_class else ""), [cfg], [0] * 8, packets, traces, [0] * 8, ns)
    g.facts = facts
    # the width the kernels route by (rss > 23: the 32-bit multiply) is the stream's sample size plus one for a channel-pair
    # element: read back from what was written -- the element tag in the packet's first three bits, the stream configuration
    assert all(p[0] >> 5 == (1 if stereo else 0) for p in packets) and cfg[1] + (packets[0][0] >> 5) == rss
    assert rss == {(False, False): 16, (True, False): 17, (False, True): 24, (True, True): 25}[(bool(stereo), bool(is24))]
    if kind == "drift":
        assert facts["peak"] > 32768, facts        # some coefficient left the int16 range it was read in
    if kind == "flat_and_tie":
        assert facts["ties"] > 0 and facts["flat"] > 0, facts
    if kind == "uniform":                          # the residuals span the rss range: its outermost 16th on either side is met
        assert facts["lo"] < -top + (top >> 4) and facts["hi"] > top - (top >> 4), facts
    if order_class:                                # the routing facts: every order lies in its class, and the edges of the class are met
        lo, hi = FIR_CLASS_ORDERS[order_class]
        plain_orders = [o for o, sp in facts["orders"] if not sp]
        assert all(lo <= o <= hi for o in plain_orders), facts
        assert [o for o, sp in facts["orders"] if sp] == ([31, 0] if order_class == "second_launch" and kind in FIR_SPECIAL_KINDS else [])
        if order_class == "first_launch":
            assert {1, 8} <= set(plain_orders)
        elif order_class == "two_taps":
            assert 16 in plain_orders and any(8 < o < 16 for o in plain_orders) and any(o <= 8 for o in plain_orders)
        if kind != "warmup":                       # every stream as long as the others: chunks 1.. run the steady-state step
            assert set(ns) == {160}
    return g


def fir_blocks(kind, order_class=None):
    if order_class:
        return range(3) if kind == "warmup" else range(2)
    return range(12) if kind == "warmup" else range(4)


def embed_filler(stereo, is24):
    """Group.embed's filler: a warm-up group (order 30, one to eight frames per packet) of the usual stream configuration"""
    return build_fir("warmup", stereo, is24, 5)


@functools.lru_cache(maxsize=None)
def build(name, stereo, is24, oc):
    return CASES[name](stereo, is24, oc)


@functools.lru_cache(maxsize=None)
def build_fir(kind, stereo, is24, block, order_class=None):
    return fir_group(kind, stereo, is24, block, order_class)
