"""The paired kernel: decode_batch_device on resident packets remembers where channel B of a two-channel
packet starts, and a later call decodes both channels of a packet side by side from that start, which it checks against where
channel A ended.  Every case decodes a batch twice on one context -- cold, then from the remembered starts -- and compares both
calls with the CPU oracle bit for bit (samples, return value, sample count, status); the counters say which way the packets went.

The batches are a few packets of at most 100 frames: a workgroup of the paired kernel takes 4 packets, a flag of the launch behind
it covers 8, so 1, 3, 4, 5 and 9 packets are a lone packet, a group that is not full, one workgroup, one and a bit, and a second
flag; frame lengths around the 32-sample chunk sit side by side in a group.  What the paired kernel must refuse (orders above 8,
more than 23 bits, a wrong start) sits in the second group of 4 of a batch of 9, next to groups it takes.
"""
import numpy as np
import pytest

import tier_cases as tc
from test_decode_into import Dev, torch  # noqa: F401  (torch: a fixture)
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

LENGTHS = [100, 1, 31, 32, 33]
CANARY = -0x5A5A5A5B
CFG16 = (4096, 16, 40, 10, 14, 2)
CFG24 = (4096, 24, 40, 10, 14, 2)


@pytest.fixture(scope="module")
def pkg(torch):
    import alac.net_amd as p

    p.lib()
    return p


def mixed(synth, n, **kw):
    """n packets, 16 bit: two-channel, one-channel and uncompressed ones mixed, the frame lengths of LENGTHS in turn."""
    d = synth.packet_descs(n, **kw)
    idx = np.arange(n)
    d["n"] = np.array(LENGTHS)[idx % len(LENGTHS)]
    d["stereo"] = np.where(idx % 4 == 1, 0, 1)
    d["escape"] = np.where(idx % 4 == 3, 1, 0)
    d["mix_weight"] = idx % 2
    d["pred_order"][:, 0] = 1 + idx % 8
    d["pred_order"][:, 1] = 8 - idx % 8
    return d


def batch_of(synth, d, stream_cfgs=(CFG16,), cfg_idx=None, seed=7):
    b = synth.make_batch(d, synth.default_signal(seed))
    b.update(stream_cfgs=list(stream_cfgs), cfg_idx=cfg_idx)
    b["slot_ints"] = max(int(b["slot_ints"]), 2 * int(d["n"].max()))
    return b


def reference(oracle, b):
    return oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"],
                               n_threads=4)


def decode(torch, ctx, d, slot_ints, stream=None):
    dev = torch.device("cuda", 0)
    pcm = torch.full((d.n, slot_ints), CANARY, dtype=torch.int32, device=dev)
    ob, os_, st = (torch.full((d.n,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        ctx.decode_batch_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, pcm, slot_ints, ob, os_, st, stream=s.cuda_stream)
    return pcm, ob, os_, st


def host(torch, got):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got)


def cold_then_warm(torch, pkg, oracle, b, paired_some=True):
    """Two calls on one context, both exact; the first finds no remembered start, the second decodes paired."""
    ref = reference(oracle, b)
    d = Dev(torch, b)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        assert ctx.pairing_stats() == (0, 0, 0)
        assert_same(host(torch, decode(torch, ctx, d, b["slot_ints"])), ref, b["stream_cfgs"], b["cfg_idx"])
        cold = ctx.pairing_stats()
        print("cold", cold)
        assert cold[0] == 0 and cold[1] > 0 and cold[2] == 0
        assert_same(host(torch, decode(torch, ctx, d, b["slot_ints"])), ref, b["stream_cfgs"], b["cfg_idx"])
        warm = ctx.pairing_stats()
        print("warm", warm)
        assert warm[2] == 0
        if paired_some:
            assert warm[0] > 0
    return ref


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_two_channel_one_channel_and_uncompressed_packets(torch, pkg, oracle, synth, n):
    ref = cold_then_warm(torch, pkg, oracle, batch_of(synth, mixed(synth, n)))
    assert (ref[3] == 0).all()


def test_a_group_with_an_order_the_paired_kernel_does_not_take(torch, pkg, oracle, synth):
    d = mixed(synth, 9)
    d["pred_order"][6, 1] = 12
    cold_then_warm(torch, pkg, oracle, batch_of(synth, d))


def test_two_stream_configs_and_a_packet_of_more_than_23_bits(torch, pkg, oracle, synth):
    # 24-bit two-channel packets: two with a shift byte (17 bits with the mid/side bit: taken), and packet 4 without (25 bits: its
    # workgroup leaves its four packets)
    d = mixed(synth, 9)
    is24 = np.zeros(9, dtype=bool)
    is24[[2, 4, 6]] = True
    assert d["stereo"][[2, 4, 6]].all() and not d["escape"][[2, 4, 6]].any()
    d["sample_size"] = np.where(is24, 24, 16)
    d["ub"] = np.where(is24, 1, 0)
    d["ub"][4] = 0
    cold_then_warm(torch, pkg, oracle, batch_of(synth, d, (CFG16, CFG24), is24.astype(np.uint16)))


def test_a_truncated_packet(torch, pkg, oracle, synth):
    b = batch_of(synth, mixed(synth, 9))
    b["sizes"][4] = b["sizes"][4] // 2       # (packet 4: two channels, 33 frames)
    ref = cold_then_warm(torch, pkg, oracle, b)
    assert ref[3][4] == 5 and (np.delete(ref[3], 4) == 0).all()


@pytest.mark.parametrize("name", ["g", "i", "f_ends"])
def test_zero_runs_and_escape_codes_written_by_hand(torch, pkg, oracle, name):
    b = tc.build(name, True, False, "first_launch").batch()
    ref = reference(oracle, b)
    assert ref[3].tolist() == b["status"]
    cold_then_warm(torch, pkg, oracle, b)


def test_a_wrong_start_is_refused(torch, pkg, oracle, synth):
    b = batch_of(synth, mixed(synth, 9))
    ref = reference(oracle, b)
    d = Dev(torch, b)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        host(torch, decode(torch, ctx, d, b["slot_ints"]))
        ctx.pairing_shift_starts()
        before = ctx.pairing_stats()
        assert_same(host(torch, decode(torch, ctx, d, b["slot_ints"])), ref, b["stream_cfgs"], b["cfg_idx"])
        after = ctx.pairing_stats()
        print(before, after)
        assert after[2] > before[2] and after[0] == before[0]
        # the launch behind remembered the right starts again
        assert_same(host(torch, decode(torch, ctx, d, b["slot_ints"])), ref, b["stream_cfgs"], b["cfg_idx"])
        assert ctx.pairing_stats()[0] > after[0]


def test_packets_rewritten_in_place(torch, pkg, oracle, synth):
    # two sets of packets at the same offsets with the same sizes (the longer of the two: what lies behind a packet's end tag is
    # not read), the second written over the first between two calls.  Packet 0 of the second set is the first set's with bytes
    # in the middle of channel A's Rice stream inverted: its tag (address, size, first 16 bytes) still fits and its remembered
    # start does not -- the check has to refuse it; packets 1..3 (its workgroup) stay, packets 4..8 differ from the first byte on
    desc = mixed(synth, 9)
    b1, b2 = batch_of(synth, desc, seed=7), batch_of(synth, desc, seed=8)
    sizes = np.maximum(b1["sizes"], b2["sizes"])
    stride = (int(sizes.max()) + 15) // 16 * 16 + 3         # (not a multiple of 16: the packets start at every alignment)
    offsets = (np.arange(9) * stride).astype(np.uint64)
    for b in (b1, b2):
        blob = np.zeros(9 * stride + 16, dtype=np.uint8)
        for k in range(9):
            o, s = int(b["offsets"][k]), int(b["sizes"][k])
            blob[int(offsets[k]):int(offsets[k]) + s] = b["blob"][o:o + s]
        b.update(blob=blob, offsets=offsets, sizes=sizes)
    b2["blob"][:4 * stride] = b1["blob"][:4 * stride]       # (the paired kernel's first workgroup: every tag fits)
    b2["blob"][48:56] ^= 0xFF
    assert desc["stereo"][0] and int(b1["sizes"][0]) > 200 and np.array_equal(b1["blob"][:16], b2["blob"][:16])
    ref1, ref2 = reference(oracle, b1), reference(oracle, b2)
    assert (ref1[3] == 0).all() and (ref2[3][1:] == 0).all() and not np.array_equal(ref1[0][0], ref2[0][0])
    d = Dev(torch, b1)
    with pkg.AlacGpuContext(b1["stream_cfgs"]) as ctx:
        for _ in range(2):
            assert_same(host(torch, decode(torch, ctx, d, b1["slot_ints"])), ref1, b1["stream_cfgs"], None)
        before = ctx.pairing_stats()
        d.blob[:b2["blob"].size] = torch.from_numpy(b2["blob"]).to(d.blob.device)
        assert_same(host(torch, decode(torch, ctx, d, b1["slot_ints"])), ref2, b1["stream_cfgs"], None)
        after = ctx.pairing_stats()
        print(before, after)
        assert after[2] == before[2] + 1 and after[1] > before[1]        # packet 0 refused by the check, others not found
        assert_same(host(torch, decode(torch, ctx, d, b1["slot_ints"])), ref2, b1["stream_cfgs"], None)


def test_two_streams_share_a_context(torch, pkg, oracle, synth):
    ba, bb = batch_of(synth, mixed(synth, 9), seed=3), batch_of(synth, mixed(synth, 5), seed=4)
    ra, rb = reference(oracle, ba), reference(oracle, bb)
    da, db = Dev(torch, ba), Dev(torch, bb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with pkg.AlacGpuContext(ba["stream_cfgs"]) as ctx:
        for _ in range(3):      # cold, then warm, then warm again: both streams in flight at once every time
            ga, gb = decode(torch, ctx, da, ba["slot_ints"], sa), decode(torch, ctx, db, bb["slot_ints"], sb)
            assert_same(host(torch, ga), ra, ba["stream_cfgs"], None)
            assert_same(host(torch, gb), rb, bb["stream_cfgs"], None)
        assert ctx.pairing_stats()[0] > 0


def test_switched_off(torch, pkg, oracle, synth):
    b = batch_of(synth, mixed(synth, 9))
    ref = reference(oracle, b)
    d = Dev(torch, b)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        ctx.set_pairing(False)
        for _ in range(2):
            assert_same(host(torch, decode(torch, ctx, d, b["slot_ints"])), ref, b["stream_cfgs"], None)
        assert ctx.pairing_stats() == (0, 0, 0)


def test_a_context_whose_starts_keep_being_wrong_stops_pairing(torch, pkg, oracle, synth):
    b = batch_of(synth, mixed(synth, 9))
    ref = reference(oracle, b)
    d = Dev(torch, b)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        host(torch, decode(torch, ctx, d, b["slot_ints"]))
        for _ in range(40):     # (the context looks at its counters every 16 paired launches)
            ctx.pairing_shift_starts()
            got = decode(torch, ctx, d, b["slot_ints"])
        assert_same(host(torch, got), ref, b["stream_cfgs"], None)
        stopped = ctx.pairing_stats()
        print(stopped)
        assert stopped[0] == 0 and 0 < stopped[2] < 40 * 9
        for _ in range(2):
            assert_same(host(torch, decode(torch, ctx, d, b["slot_ints"])), ref, b["stream_cfgs"], None)
        assert ctx.pairing_stats() == stopped


def test_a_context_that_never_finds_its_packets_stops_the_paired_launch(torch, pkg, oracle, synth):
    # packets at an address the context has not seen in every call: after a window of such calls (16) no paired launch looks for them
    b = batch_of(synth, mixed(synth, 9))
    ref = reference(oracle, b)
    d = Dev(torch, b)
    copies = [d.blob.clone() for _ in range(40)]
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        seen = []
        for c in copies:
            d.blob = c
            got = host(torch, decode(torch, ctx, d, b["slot_ints"]))
            seen.append(ctx.pairing_stats())
        assert_same(got, ref, b["stream_cfgs"], None)
        print(seen[0], seen[-1])
        assert all(s[0] == 0 and s[2] == 0 for s in seen)
        assert seen[0][1] == 5 and seen[-1] == seen[-2] == seen[20] and seen[-1][1] <= 5 * 20
