"""Directed GPU cases for the entropy wave's tiers and the FIR waves: packets written symbol by symbol (tests/rice_writer.py,
tests/tier_cases.py) so that a stream sits exactly on an edge of the speculative units -- next to chosen neighbours -- instead of
wherever an encoder's output happens to land.  Every builder asserts its premise from the writer's trace before anything runs;
the GPU result is compared with the CPU oracle bit for bit (samples, return value, sample count, status) in all four
arrangements, with LPC orders of all three classes, mono and stereo, 16 and 24 bit.  Cases f, k and l -- packets that end early,
zero runs past the end, the highest bit rates -- also go through decode_into_device (float32, planar).

Case k (59 and 34 bits per sample against the ring's top-up) is the one most likely to do more than mismatch.  Before a change
to the entropy wave is run through this file, run it alone, once, in a process and under a time limit of its own:
    timeout 200 python -m pytest tests/test_entropy_tiers.py -m gpu -x -k "k_59 or k_34"
and go on to the rest only when that came back clean.  (Its place at the head of the parameter list is a convenience, not a guard.)

These batches have 16 packets, mixed FIR orders and the plain builds.  tests/test_fir_steps.py runs the FIR groups with every order
inside one class -- one build of the steady-state FIR step per group -- and embeds them and the cases of this file in launches
of 2056 packets, where orders above 16 take the four-taps-per-lane step; tests/test_window_tiers.py sends the store-pattern
cases through the window builds (decode_window_into_device) with directed skips.
"""
import numpy as np
import pytest

import tier_cases as tc
from test_decode_into import Dev, check, decode_into, expected, gapless, torch  # noqa: F401  (torch: a fixture)
from test_gpu_parity import arrangement, assert_same  # noqa: F401  (arrangement: the fixture of the four builds)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(torch):
    # (torch takes the device before the library does, as in tests/test_decode_into.py)
    import alac.net_amd as p

    p.lib()
    return p


def run_group(pkg, oracle, g):
    b = g.batch()
    with pkg.AlacGpuContext(b["stream_cfgs"], device=0) as ctx:
        got = ctx.decode_batch(b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"])
    ref = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"],
                              n_threads=8)
    assert ref[3].tolist() == b["status"], f"case {g.name}: oracle status {ref[3].tolist()}"
    try:
        assert_same(got, ref, b["stream_cfgs"], b["cfg_idx"])
    except AssertionError as e:
        raise AssertionError(f"case {g.name} (packets in the order {b['order']}): {e}") from None


@pytest.mark.parametrize("oc", tc.ORDER_CLASSES)
@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("name", ["k_59", "k_34"] + [c for c in tc.CASES if not c.startswith("k_")])
def test_entropy_case(pkg, oracle, name, stereo, is24, oc):
    run_group(pkg, oracle, tc.build(name, stereo, is24, oc))


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("kind", tc.FIR_KINDS)
def test_fir_case(pkg, oracle, kind, stereo, is24):
    for block in tc.fir_blocks(kind):
        run_group(pkg, oracle, tc.build_fir(kind, stereo, is24, block))


@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("name", ["k_59", "k_34", "f", "f_ends", "l"])
def test_store_pattern_cases_into_device_float32_planar(torch, pkg, oracle, name, stereo, is24):
    # the packets one behind the other in a planar float32 tensor, canaries around them: what a packet that ends early, or a zero
    # run that goes past the packet's end, leaves alone counts as much as what it stores
    g = tc.build(name, stereo, is24, tc.ORDER_CLASSES[(stereo + 2 * is24) % 3])
    b = g.batch()
    channels = g.cfgs[0][5]
    ref = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"],
                              channels * max(c[0] for c in g.cfgs), n_threads=8)
    assert ref[3].tolist() == b["status"]
    first, frames, total = gapless(ref)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        out, os_, st, _ = decode_into(torch, ctx, Dev(torch, b), first, frames, "float32", "planar", channels, total * channels, total)
        torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), ref[3]) and np.array_equal(os_.cpu().numpy(), ref[2])
    check(torch, out, expected(b, ref, first, frames, "float32", "planar", channels, total * channels, total, ref[3]))
