"""The paired kernel's 8-packet form (alac_decode_ab_pair_dense_kernel): 8 packets x 2 channels per workgroup
on the dense layout.  Every case forces that form (ALACGPU_PAIR_DENSE=1, read when a context is created: batches this small would
take the 4-packet form otherwise), decodes a batch cold and from the remembered starts, and compares samples, return value,
sample count, status and the canary behind each packet's samples with the CPU oracle.

A workgroup takes 8 packets and a flag of the launch behind it covers the same 8, so 1, 7, 8, 9, 15, 16 and 17 packets are a lone
packet, a group one short, one workgroup, one and a bit, and so on; frame lengths around the 32-sample chunk sit side by side.
"""
import numpy as np
import pytest

from test_decode_into import Dev, torch  # noqa: F401  (torch: a fixture)
from test_pairing import CANARY, CFG16, CFG24, assert_same, batch_of, cold_then_warm, decode, host, mixed, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(torch):
    import alac.net_amd as p

    p.lib()
    return p


@pytest.fixture(autouse=True)
def dense_form(monkeypatch):
    monkeypatch.setenv("ALACGPU_PAIR_DENSE", "1")


def check(got, ref, b):
    """assert_same, and nothing written behind a decoded packet's samples"""
    assert_same(got, ref, b["stream_cfgs"], b["cfg_idx"])
    pcm, samples, status = got[0], ref[2], ref[3]
    for k in np.nonzero(status == 0)[0]:
        nc = int(b["stream_cfgs"][0 if b["cfg_idx"] is None else int(b["cfg_idx"][k])][5])
        assert (pcm[k, int(samples[k]) * nc:] == CANARY).all(), f"packet {k}: stores behind its samples"


def calls(torch, pkg, b, n_calls, ref=None):
    """n_calls calls on one context: [(outputs, counters after the call)], every call checked against `ref`"""
    d = Dev(torch, b)
    seen = []
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        for _ in range(n_calls):
            got = host(torch, decode(torch, ctx, d, b["slot_ints"]))
            if ref is not None:
                check(got, ref, b)
            seen.append((got, ctx.pairing_stats()))
    return seen


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17])
def test_ragged_groups(torch, pkg, oracle, synth, n):
    b = batch_of(synth, mixed(synth, n))
    ref = cold_then_warm(torch, pkg, oracle, b)          # (warm: hits > 0, wrong == 0)
    assert (ref[3] == 0).all()
    calls(torch, pkg, b, 2, ref)                         # (the same two calls with the canary looked at)


def last_of_eight_compressed(synth):
    d = mixed(synth, 16)
    d["escape"][7] = 0
    assert d["stereo"][7]
    return d


@pytest.mark.parametrize("how", ["order 12", "25 bits"])
def test_the_last_packet_of_a_group_disqualifies(torch, pkg, oracle, synth, how):
    d = last_of_eight_compressed(synth)
    if how == "order 12":
        d["pred_order"][7, 1] = 12
        b = batch_of(synth, d)
    else:
        is24 = np.zeros(16, dtype=bool)
        is24[7] = True
        d["sample_size"] = np.where(is24, 24, 16)      # (24 bits without a shift byte, and the mid/side bit: 25)
        b = batch_of(synth, d, (CFG16, CFG24), is24.astype(np.uint16))
    ref = reference(oracle, b)
    (_, cold), (_, warm) = calls(torch, pkg, b, 2, ref)
    print(cold, warm)
    # the first group leaves, the second pairs: its compressed two-channel packets are 8, 10, 12 and 14
    assert cold[0] == 0 and 0 < warm[0] <= 4 and warm[2] == 0


def test_one_wrong_start_in_a_group(torch, pkg, oracle, synth):
    # packet 5 of 8 replaced in place by a packet of the same size with the same first 16 bytes whose channel A ends elsewhere
    # (bytes in the middle of A's Rice stream inverted): its tag fits, its remembered start does not
    desc = mixed(synth, 8)
    desc["stereo"][5] = 1
    b1 = batch_of(synth, desc)
    o5, s5 = int(b1["offsets"][5]), int(b1["sizes"][5])
    assert s5 > 120
    b2 = dict(b1, blob=b1["blob"].copy())
    b2["blob"][o5 + 48:o5 + 56] ^= 0xFF
    ref1, ref2 = reference(oracle, b1), reference(oracle, b2)
    assert (ref1[3] == 0).all() and not np.array_equal(ref1[0][5], ref2[0][5])
    two = int(((desc["stereo"] == 1) & (desc["escape"] == 0)).sum())
    d = Dev(torch, b1)
    with pkg.AlacGpuContext(b1["stream_cfgs"]) as ctx:
        for _ in range(2):
            check(host(torch, decode(torch, ctx, d, b1["slot_ints"])), ref1, b1)
        before = ctx.pairing_stats()
        assert 0 < before[0] <= two
        d.blob[:b2["blob"].size] = torch.from_numpy(b2["blob"]).to(d.blob.device)
        check(host(torch, decode(torch, ctx, d, b1["slot_ints"])), ref2, b1)
        after = ctx.pairing_stats()
        print(before, after)
        assert after[2] == before[2] + 1 and after[0] == before[0] and after[1] == before[1]
        check(host(torch, decode(torch, ctx, d, b1["slot_ints"])), ref2, b1)
        again = ctx.pairing_stats()
        assert again[0] > after[0] and again[2] == after[2]


@pytest.fixture(scope="module")
def long_batch(synth, oracle):
    b = batch_of(synth, synth.packet_descs(16))         # 16 two-channel packets of 4096 frames, order 8, mix weight 1
    return b, reference(oracle, b)


def test_full_length_chains(torch, pkg, long_batch):
    b, ref = long_batch
    assert (ref[3] == 0).all() and (ref[2] == 4096).all()
    (_, cold), (_, warm) = calls(torch, pkg, b, 2, ref)
    assert cold[0] == 0 and 0 < warm[0] <= 16 and warm[2] == 0


def test_two_streams_share_a_context(torch, pkg, long_batch):
    b, ref = long_batch
    d = Dev(torch, b)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    dev = torch.device("cuda", 0)
    torch.cuda.synchronize()
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        for _ in range(3):      # cold, then warm twice: both streams in flight at once every time
            # (the canaries are written on the current stream, which the two streams do not wait for: both sets first, then a
            # synchronize, then the two calls)
            outs = [(torch.full((d.n, b["slot_ints"]), CANARY, dtype=torch.int32, device=dev),
                     *(torch.full((d.n,), -1, dtype=torch.int32, device=dev) for _ in range(3))) for _ in range(2)]
            torch.cuda.synchronize()
            for s, (pcm, ob, os_, st) in zip((sa, sb), outs):
                with torch.cuda.stream(s):
                    ctx.decode_batch_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, pcm, b["slot_ints"], ob, os_, st, stream=s.cuda_stream)
            for got in outs:
                check(host(torch, got), ref, b)
        assert ctx.pairing_stats()[0] > 0


def test_counters_count_packets(torch, pkg, oracle, synth):
    d = synth.packet_descs(11)
    d["n"] = 40
    b = batch_of(synth, d)
    (_, cold), (_, warm), (_, again) = calls(torch, pkg, b, 3, reference(oracle, b))
    assert cold == (0, 11, 0) and warm == (11, 11, 0) and again == (22, 11, 0)
