"""The GPU encoder's analysis pass against the policy reference (encode_ref.py): LPC, mix weight and escape choices byte for
byte over tones, DC, mirrored channels, noise and an escape-threshold sweep; frame counts at the LDS chunk edges; batches of
more than one launch round with mixed cfgs; every PCM layout; off-range samples; kb multiples of 32; one context shared by
calls on two streams."""
import io

import numpy as np
import pytest

import encode_ref as er
import test_encode as te

pytestmark = pytest.mark.gpu

CANARY = te.CANARY
MAX_NONFIRM = 3   # per test: non-firm packets are rare (none met on the test signals); each may differ by 1 in a coefficient


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.device_count() > 0
    t.cuda.set_device(0)
    return t


@pytest.fixture(scope="module")
def pkg():
    import alac.net_amd as p

    p.lib()
    return p


def run(torch, pkg, pcm, C_, cfgs, firsts, frames, cfg_idx=None, layout="planar", plane_stride=0, slot=None, ctx=None,
        stream=None, sync=True):
    """One encode_device call on device tensor pcm; returns (packets, status, raw slots, slot, sizes) -- or, with sync False,
    the device tensors (d_packets, d_sizes, d_status, slot) for the caller to read after it has synchronised."""
    n = len(frames)
    ci = np.zeros(n, np.int16) if cfg_idx is None else np.asarray(cfg_idx).astype(np.int16)
    if slot is None:
        slot = max(pkg.encode_max_packet_bytes(min(c[0], 16384), c[1], C_) for c in cfgs)
    d_packets = torch.full((n * slot,), CANARY, dtype=torch.uint8, device="cuda")
    d_sizes = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    args = (pcm, C_, torch.from_numpy(np.asarray(firsts, np.int64)).cuda(), torch.from_numpy(np.asarray(frames, np.int32)).cuda(),
            torch.from_numpy(ci).cuda(), n, d_packets, slot, d_sizes, d_st)
    s = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()   # the argument tensors are ready before a call on another stream reads them
    if ctx is None:
        with pkg.AlacGpuContext(cfgs) as c:
            c.encode_device(*args, layout=layout, plane_stride=plane_stride, stream=s.cuda_stream)
            torch.cuda.synchronize()
    else:
        ctx.encode_device(*args, layout=layout, plane_stride=plane_stride, stream=s.cuda_stream)
        if not sync:   # (the argument tensors go along: they must outlive the call)
            return (d_packets, d_sizes, d_st, slot), args
        torch.cuda.synchronize()
    return unpack(d_packets, d_sizes, d_st, slot)


def unpack(d_packets, d_sizes, d_st, slot):
    raw, sizes, st = d_packets.cpu().numpy(), d_sizes.cpu().numpy(), d_st.cpu().numpy()
    return [raw[p * slot:p * slot + int(sizes[p])].tobytes() for p in range(len(st))], st, raw, slot, sizes


def planar_of(parts):
    """[n_p, C] arrays back to back: planar [C, T], firsts, frames."""
    frames = np.array([len(p) for p in parts], np.int64)
    firsts = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(parts).T), firsts, frames


class Tally:
    """Compares GPU packets with reference packets: firm ones byte for byte; non-firm ones counted, bounded, and allowed to
    differ only by 1 in header coefficients (same escape flag and mix weight); the escape margins seen."""

    def __init__(self, synth):
        self.synth, self.nonfirm, self.margins, self.packets = synth, 0, [], 0

    def check(self, pkt, pcm, cfg, exact="auto", what=""):
        ref = er.reference_packet(self.synth, pcm, cfg, exact=exact)
        self.packets += 1
        if ref.margin is not None:
            self.margins.append(ref.margin)
        if ref.firm:
            assert pkt == ref.packet, f"{what}: packet differs from the policy reference (weight {ref.weight}, escape " \
                                      f"{ref.escape}, margin {ref.margin})"
        else:
            self.nonfirm += 1
            if pkt != ref.packet:
                g, _, _ = te.recipe(self.synth, pkt, cfg)
                r, _, _ = te.recipe(self.synth, ref.packet, cfg)
                assert int(g["escape"][0]) == int(r["escape"][0]) == 0, what
                assert int(g["mix_weight"][0]) == int(r["mix_weight"][0]), what
                assert np.abs(g["coefs"].astype(np.int64) - r["coefs"].astype(np.int64)).max() <= 1, what
            # and it must still be the CPU encoder's packet for its own recipe
            te.check_twin(self.synth, [pkt], np.ascontiguousarray(ref.samples.T.astype(np.int32)), [0], [len(pcm)], [cfg])
        return ref

    def done(self):
        assert self.nonfirm <= MAX_NONFIRM, self.nonfirm
        print(f"[encode policy] {self.packets} packets, {self.nonfirm} non-firm")


def signals(synth, ss, C_):
    """(name, [n, C] int32) packets: synth signals, tones, DC with silence, mirrored / silent channels, full-scale noise."""
    rng = np.random.default_rng(ss * 10 + C_)
    lo, hi = er.sample_range(ss)
    n, i = 4096, np.arange(4096)
    out = []
    for seed in range(4):
        for p in range(3):
            out.append((f"synth{seed}.{p}", synth.make_pcm(synth.default_signal(500 + seed), p, ss, C_, n).reshape(-1, C_)))
    for j in range(3):
        f = rng.uniform(0.001, 0.3)
        tone = np.stack([np.round(hi * 0.7 * np.sin(f * i + j)), np.round(hi * 0.4 * np.sin(f * i + 1))], 1)
        dc = np.stack([np.full(n, rng.integers(lo, hi)), np.full(n, rng.integers(lo, hi))], 1)
        a = int(rng.integers(0, 3000))
        dc[a:a + 1000] = 0
        out += [(f"tone{j}", tone[:, :C_]), (f"dc{j}", dc[:, :C_])]
    x = np.round(0.3 * hi * np.sin(0.013 * i) + 0.1 * hi * np.sin(0.21 * i + 1) + rng.normal(0, hi / 800, n))
    if C_ == 2:
        out += [("l=r", np.stack([x, x], 1)), ("l=-r", np.stack([x, -x], 1)), ("r=0", np.stack([x, 0 * x], 1)),
                ("l=0", np.stack([0 * x, x], 1))]
    out.append(("noise", rng.integers(lo, hi + 1, (n, C_))))
    return [(k, np.clip(v, lo, hi).astype(np.int32)) for k, v in out]


def sweep(ss, C_, count=96, n=96):
    """Gaussian noise whose level climbs across the escape threshold, one short packet per level."""
    rng = np.random.default_rng(ss * 10 + C_)
    lo, hi = er.sample_range(ss)
    return [np.clip(np.round(rng.normal(0, 2 ** (ss - 5.5 + 2 * k / (count - 1)), (n, C_))), lo, hi).astype(np.int32)
            for k in range(count)]


@pytest.mark.parametrize("ss,C_", [(16, 2), (24, 2), (16, 1), (24, 1)])
def test_policy_byte_for_byte(torch, pkg, synth, ss, C_):
    sig = signals(synth, ss, C_)
    sw = sweep(ss, C_)
    parts = [v for _, v in sig] + sw
    planar, firsts, frames = planar_of(parts)
    cfg = (4096, ss, 40, 10, 14, C_)
    pk, st, _, _, _ = run(torch, pkg, torch.from_numpy(planar).cuda(), C_, [cfg], firsts, frames, plane_stride=planar.shape[1])
    assert (st == 0).all()
    t = Tally(synth)
    refs = [t.check(pk[p], parts[p], cfg, what=(sig[p][0] if p < len(sig) else f"sweep{p - len(sig)}"))
            for p in range(len(parts))]
    named = {k: refs[p] for p, (k, _) in enumerate(sig)}
    assert named["noise"].escape
    if C_ == 2:   # L == R: weights 1..4 tie exactly, the smallest wins; L == -R: A_2 is silent
        assert named["l=r"].weight == 1 and len({named["l=r"].nbits[w] for w in (1, 2, 3, 4)}) == 1
        assert named["l=-r"].weight == 2
    m = np.array([r.margin for r in refs[len(sig):]])
    assert (m <= 0).any() and (m > 0).any(), m
    print(f"[encode policy] sweep ss {ss} C {C_}: {(m <= 0).sum()} escape, {(m > 0).sum()} compressed, "
          f"{(m == 0).sum()} at margin 0, smallest |margin| {np.abs(m).min()} bytes")
    t.done()


def oracle_roundtrip(oracle, pk, cfgs, frames, cfg_idx, planar_ints, firsts):
    """The C oracle decodes every packet back to its canonical samples."""
    C_ = cfgs[0][5]
    n = len(pk)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum([((len(x) + 15) // 16) * 16 for x in pk])[:-1]
    blob = np.zeros(int(offs[-1]) + len(pk[-1]) + 64, np.uint8)
    for o, x in zip(offs, pk):
        blob[int(o):int(o) + len(x)] = np.frombuffer(x, np.uint8)
    smax = max(min(c[0], 16384) for c in cfgs)
    ref, _, osm, rst = oracle.decode_batch(oracle.make_cfgs(cfgs), blob, offs, np.array([len(x) for x in pk], np.uint32),
                                           cfg_idx, smax * C_, n_threads=8)
    assert (rst == 0).all() and (osm == np.asarray(frames)).all()
    for p in range(n):
        got = ref[p, :frames[p] * C_].reshape(-1, C_).T
        assert np.array_equal(got, planar_ints[:, firsts[p]:firsts[p] + frames[p]]), p


EDGES = [1, 2, 8, 9, 10, 511, 512, 513, 519, 520, 521, 1024, 1025, 4095, 4096, 16383, 16384]


@pytest.mark.parametrize("ss,C_", [(16, 2), (24, 1)])
def test_chunk_edges(torch, pkg, synth, oracle, ss, C_):
    """Every n at the edges of the 512-frame LDS chunks and their 8-frame halos, as a full packet (its own cfg) and as a
    hassize packet (max_samples_per_frame 16384), all in one call through cfg_idx."""
    cfgs = [(n, ss, 40, 10, 14, C_) for n in EDGES]          # cfg k: packets of EDGES[k] frames are full
    sig = synth.default_signal(77)
    parts, ci = [], []
    for k, n in enumerate(EDGES):
        for full in (True, False):
            if n == 16384 and not full:
                continue
            parts.append(synth.make_pcm(sig, len(parts), ss, C_, n).reshape(-1, C_))
            ci.append(k if full else len(EDGES) - 1)
    planar, firsts, frames = planar_of(parts)
    pk, st, _, _, _ = run(torch, pkg, torch.from_numpy(planar).cuda(), C_, cfgs, firsts, frames, cfg_idx=ci,
                          plane_stride=planar.shape[1])
    assert (st == 0).all()
    t = Tally(synth)
    for p, part in enumerate(parts):
        cfg = cfgs[ci[p]]
        ref = t.check(pk[p], part, cfg, what=f"n {len(part)} cfg {cfg[0]}")
        assert te.recipe(synth, pk[p], cfg)[1] == (len(part) != cfg[0])   # hassize
        assert not ref.escape or len(part) < 500
    t.done()
    oracle_roundtrip(oracle, pk, cfgs, frames, np.asarray(ci, np.uint16), planar, firsts)


def test_multi_round_batch(torch, pkg, synth):
    """2 rounds + 3 packets in one call, cfgs mixed through cfg_idx, failing packets in the last round: every packet equals
    the same packet from calls of fewer than a round, every firm one the reference; failing slots stay untouched."""
    rnd = torch.cuda.get_device_properties(0).multi_processor_count * 16   # the C ABI's round
    n = 2 * rnd + 3
    cfgs = [(4096, 16, 40, 10, 14, 2), (1024, 24, 28, 12, 11, 2), (512, 16, 20, 4, 33, 2), (16384, 24, 48, 14, 16, 2)]
    rng = np.random.default_rng(31)
    ci = rng.integers(0, len(cfgs), n)
    frames = np.array([int(rng.integers(1, min(cfgs[c][0], 300) + 1)) for c in ci], np.int64)
    for p in range(0, n, 97):
        frames[p] = min(cfgs[ci[p]][0], 1024)                  # some full packets
    T = int(frames.sum())
    firsts = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64)
    x = np.arange(T)
    planar = np.stack([np.round(9000 * np.sin(0.01 * x) + rng.normal(0, 300, T)),
                       np.round(7000 * np.sin(0.011 * x + 1) + rng.normal(0, 300, T))]).astype(np.int32)
    planar[:, rng.random(T) < 0.001] = 0
    is24 = np.array([cfgs[c][1] == 24 for c in ci])
    for p in np.nonzero(is24)[0]:                                # 24-bit packets use the whole range
        planar[:, firsts[p]:firsts[p] + frames[p]] *= 256
    bad = {n - 1: 4, n - 2: 8, n - 3: 7}                         # in the last round: bad count, out of range, bad cfg
    frames_c, firsts_c, ci_c = frames.copy(), firsts.copy(), ci.copy()
    frames_c[n - 1] = cfgs[ci[n - 1]][0] + 1
    firsts_c[n - 2] = T - 1
    frames_c[n - 2] = 2
    ci_c[n - 3] = len(cfgs)
    d_pcm = torch.from_numpy(planar).cuda()
    pk, st, raw, slot, sizes = run(torch, pkg, d_pcm, 2, cfgs, firsts_c, frames_c, cfg_idx=ci_c, plane_stride=T)
    want_st = np.zeros(n, np.int64)
    for p, s in bad.items():
        want_st[p] = s
    assert st.tolist() == want_st.tolist()
    for p in bad:
        assert sizes[p] == 0 and (raw[p * slot:(p + 1) * slot] == CANARY).all(), p
    good = np.array([p for p in range(n) if p not in bad])
    piece = rnd // 2 + 1                                         # calls of fewer than a round each
    for a in range(0, len(good), piece):
        sel = good[a:a + piece]
        sp, sst, _, _, _ = run(torch, pkg, d_pcm, 2, cfgs, firsts[sel], frames[sel], cfg_idx=ci[sel], plane_stride=T)
        assert (sst == 0).all()
        for q, p in enumerate(sel):
            assert sp[q] == pk[p], f"packet {p} differs between one call and calls of {piece}"
    t = Tally(synth)
    for p in good:
        cfg = cfgs[ci[p]]
        t.check(pk[p], planar[:, firsts[p]:firsts[p] + frames[p]].T, cfg, what=f"packet {p}")
    t.done()


def test_layouts(torch, pkg, synth):
    """int32 / float32, planar / interleaved, and planar from a wider buffer: identical packets."""
    ss, C_ = 16, 2
    cfg = (4096, ss, 40, 10, 14, C_)
    parts = [synth.make_pcm(synth.default_signal(9), p, ss, C_, 4096).reshape(-1, C_) for p in range(5)]
    parts[-1] = parts[-1][:777]
    planar, firsts, frames = planar_of(parts)
    T = planar.shape[1]
    sc = 2.0 ** -(ss - 1)
    outs = {}
    pl = torch.from_numpy(planar).cuda()
    il = torch.from_numpy(np.ascontiguousarray(planar.T)).cuda()
    outs["i32 planar"] = run(torch, pkg, pl, C_, [cfg], firsts, frames, plane_stride=T)
    outs["i32 interleaved"] = run(torch, pkg, il, C_, [cfg], firsts, frames, layout="interleaved")
    outs["f32 planar"] = run(torch, pkg, pl.float() * sc, C_, [cfg], firsts, frames, plane_stride=T)
    outs["f32 interleaved"] = run(torch, pkg, il.float() * sc, C_, [cfg], firsts, frames, layout="interleaved")
    wide = np.full((C_, T + 300), 12345, np.int32)                 # frames outside the runs must not matter
    wide[:, 100:100 + T] = planar
    wide[:, :100] = np.random.default_rng(1).integers(-30000, 30000, (C_, 100))
    outs["i32 wide planar"] = run(torch, pkg, torch.from_numpy(wide).cuda(), C_, [cfg], firsts + 100, frames,
                                  plane_stride=T + 300)
    ref = outs["i32 planar"][0]
    for k, v in outs.items():
        assert (v[1] == 0).all(), k
        assert v[0] == ref, k
    te.check_twin(synth, ref, planar, firsts, frames, [cfg])
    # an interleaved run past src_elems / C: status 8, its slot untouched
    pk, st, raw, slot, sizes = run(torch, pkg, il, C_, [cfg], [0, T - 10, T], [100, 11, 1], layout="interleaved")
    assert st.tolist() == [0, 8, 8] and sizes[1] == sizes[2] == 0
    for p in (1, 2):
        assert (raw[p * slot:(p + 1) * slot] == CANARY).all()


def edge_packets(ss, C_):
    """The conversion table's values, int32 and float32, spread over a packet of music-like samples."""
    import test_encode_ref as ter

    ints, floats = ter.conversion_table(ss)
    lo, hi = er.sample_range(ss)
    n = 2048
    i = np.arange(n)
    base = np.round(0.2 * hi * np.sin(0.02 * i))
    out = []
    for table, dt in ((ints, np.int32), (floats, np.float32)):
        vals = np.array([v for v, _ in table], dt)
        x = (base.astype(np.int32) if dt == np.int32 else (base * 2.0 ** -(ss - 1)).astype(np.float32))
        x = np.stack([x, x[::-1]], 1)[:, :C_].copy()
        x[5:5 + 8 * len(vals):8, 0] = vals
        if C_ == 2:
            x[11:11 + 8 * len(vals):8, 1] = vals[::-1]
        out.append(x)
    return out


@pytest.mark.parametrize("ss,C_", [(16, 2), (24, 1)])
def test_off_range_input(torch, pkg, synth, oracle, ss, C_):
    """Samples off the grid or out of range: clamped and rounded as the reference converts them, decoded back exactly."""
    cfg = (4096, ss, 40, 10, 14, C_)
    t = Tally(synth)
    for x in edge_packets(ss, C_):
        planar = np.ascontiguousarray(x.T)
        pk, st, _, _, _ = run(torch, pkg, torch.from_numpy(planar).cuda(), C_, [cfg], [0], [len(x)], plane_stride=len(x))
        assert (st == 0).all()
        ref = t.check(pk[0], x, cfg, what=str(x.dtype))
        ints = np.ascontiguousarray(ref.samples.T.astype(np.int32))
        te.check_twin(synth, pk, ints, [0], [len(x)], [cfg])
        oracle_roundtrip(oracle, pk, [cfg], [len(x)], None, ints, [0])
        if x.dtype == np.float32:
            buf = io.BytesIO()
            pkg.save(buf, torch.from_numpy(planar).cuda(), 44100, sample_size=ss)
            back, _ = pkg.load(buf.getvalue(), dtype=torch.int32)
            assert np.array_equal(back.cpu().numpy(), ints)
    t.done()


@pytest.mark.parametrize("kb", [31, 32, 33, 64])
@pytest.mark.parametrize("C_", [1, 2])
def test_kb_zero_runs(torch, pkg, synth, oracle, kb, C_):
    """kb 32 or 64: a silent stretch makes every candidate unusable (escape); 31 and 33: zero runs are coded."""
    cfg = (4096, 16, 40, 10, kb, C_)
    sig = synth.default_signal(3)
    sig["silence_prob"] = 1.0
    parts = [synth.make_pcm(sig, p, 16, C_, 4096).reshape(-1, C_) for p in range(4)]
    parts.append(np.zeros((300, C_), np.int32))
    planar, firsts, frames = planar_of(parts)
    pk, st, _, _, _ = run(torch, pkg, torch.from_numpy(planar).cuda(), C_, [cfg], firsts, frames, plane_stride=planar.shape[1])
    assert (st == 0).all()
    t = Tally(synth)
    refs = [t.check(pk[p], parts[p], cfg, what=f"packet {p}") for p in range(len(parts))]
    assert all(r.escape for r in refs) == (kb % 32 == 0)
    t.done()
    oracle_roundtrip(oracle, pk, [cfg], frames, None, planar, firsts)


def test_one_context_two_streams(torch, pkg, synth):
    """Calls on two streams through one context: a small call, one larger than a round (its workspace grows behind the
    first), the small call again; each equals a fresh single call."""
    rnd = torch.cuda.get_device_properties(0).multi_processor_count * 16
    cfg = (512, 16, 40, 10, 14, 2)
    n_big = rnd + 5
    T = 512 * n_big
    x = np.arange(T)
    rng = np.random.default_rng(2)
    planar = np.stack([np.round(8000 * np.sin(0.003 * x) + rng.normal(0, 200, T)),
                       np.round(6000 * np.sin(0.005 * x) + rng.normal(0, 200, T))]).astype(np.int32)
    d_pcm = torch.from_numpy(planar).cuda()
    firsts_b, frames_b = te.split(T, 512)
    firsts_s, frames_s = firsts_b[:7] + 3, frames_b[:7] - 3
    fresh_s = run(torch, pkg, d_pcm, 2, [cfg], firsts_s, frames_s, plane_stride=T)[0]
    fresh_b = run(torch, pkg, d_pcm, 2, [cfg], firsts_b, frames_b, plane_stride=T)[0]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext([cfg]) as ctx:
        a = run(torch, pkg, d_pcm, 2, [cfg], firsts_s, frames_s, plane_stride=T, ctx=ctx, stream=s1, sync=False)
        b = run(torch, pkg, d_pcm, 2, [cfg], firsts_b, frames_b, plane_stride=T, ctx=ctx, stream=s2, sync=False)
        c = run(torch, pkg, d_pcm, 2, [cfg], firsts_s, frames_s, plane_stride=T, ctx=ctx, stream=s1, sync=False)
        torch.cuda.synchronize()
        for got, want in ((a, fresh_s), (b, fresh_b), (c, fresh_s)):
            pk, st, _, _, _ = unpack(*got[0])
            assert (st == 0).all() and pk == want
