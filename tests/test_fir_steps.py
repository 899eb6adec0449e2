"""Directed GPU cases for every build of the steady-state FIR step (alac_device.h: firb_step<T, WIDE, SPECIAL, PH, L, E>).  Which
build a group of eight packets runs on follows from its LPC orders, its width, the arrangement and the size of the launch
(alac_kernels.hip: ab_kernel_body), so the FIR groups of tests/tier_cases.py are built with every order inside one class:
    first_launch    orders 1..8: one tap per lane, the 24-bit multiply-add (rss 16 / 17) or the 32-bit one with clamps (rss 24 / 25)
    two_taps        orders 1..16 with some above 8: two taps per lane, in the second launch (the dense arrangement: the first)
    second_launch   orders 17..30 (and 31 / 0): 16 lanes per stream and two taps per lane in launches of up to
                    tc.L16_MAX_GROUPS groups, one wave with four taps per lane above that
The dense arrangement runs the one- and two-tap steps on the short queue entry (XQ8: the coefficient update from the sign mask).
A 16-packet batch never reaches the four-tap step: Group.embed puts the directed group into a launch of tc.EMBED_GROUPS groups
(at its head, in its middle and at its end, warm-up packets of a few frames everywhere else), in ONE host range -- the host
path cuts batches of 1024 packets and more in two, and either half would be back under the threshold.  The entropy cases go
through the same embedding, so that the four-tap wave also consumes the queue behind escape codes, zero runs and early ends.
Everything is compared with the CPU oracle bit for bit: samples, return value, sample count, status -- of all 2056 packets.

As in tests/test_entropy_tiers.py, case k is the one most likely to do more than mismatch; before a change to the entropy wave or
the queues is run through this file, run its embedded form alone, once, under a time limit of its own:
    timeout 300 python -m pytest tests/test_fir_steps.py -m gpu -x -k "embedded and (k_59 or k_34)"
"""
import numpy as np
import pytest

import tier_cases as tc
from test_decode_window import torch  # noqa: F401  (a fixture)
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

ARRANGEMENTS = {"auto": None, "dense": "1", "ab5": "2", "ab": "4"}      # ALACGPU_DENSE, read when a context is created
FOUR_TAP_MIN_PACKETS = 8 * tc.L16_MAX_GROUPS + 1                         # 2049: the first batch size of more than 256 groups
# the entropy cases of at most 4096 frames per packet, the two of case k first (tc.OVER_4096_FRAMES names the others, checked
# against the built groups on the CPU: building every case here would cost each collection of this file half a minute)
EMBEDDED_CASES = [(name, stereo, is24) for name in ["k_59", "k_34"] + [c for c in tc.CASES if not c.startswith("k_")]
                  for stereo, is24 in tc.VARIANTS if (name, stereo, is24) not in tc.OVER_4096_FRAMES]


@pytest.fixture(scope="module")
def pkg(torch):
    # (torch takes the device before the library does, as in tests/test_entropy_tiers.py)
    import alac.net_amd as p

    p.lib()
    return p


def arrange(monkeypatch, arrangement, one_range=False):
    if ARRANGEMENTS[arrangement] is None:
        monkeypatch.delenv("ALACGPU_DENSE", raising=False)
    else:
        monkeypatch.setenv("ALACGPU_DENSE", ARRANGEMENTS[arrangement])
    if one_range:
        monkeypatch.setenv("ALACGPU_HOST_CHUNKS", "1")
    else:
        monkeypatch.delenv("ALACGPU_HOST_CHUNKS", raising=False)


_REF = {}      # the oracle's verdict per batch, shared by the arrangements (read only)


def run_batch(pkg, oracle, key, make, what, big=False):
    if key not in _REF:
        if big or len(_REF) >= 8:
            _REF.clear()   # (an embedded batch and its output are tens of megabytes: one at a time)
        b = make()
        ref = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"],
                                  n_threads=8)
        assert ref[3].tolist() == b["status"], f"{what}: oracle status {ref[3].tolist()}"
        _REF[key] = (b, ref)
    b, ref = _REF[key]
    with pkg.AlacGpuContext(b["stream_cfgs"], device=0) as ctx:
        got = ctx.decode_batch(b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], b["slot_ints"])
    try:
        assert_same(got, ref, b["stream_cfgs"], b["cfg_idx"])
    except AssertionError as e:
        raise AssertionError(f"{what} (the group's packets as (batch index, packet): {b['order']}): {e}") from None


def two_groups(first, second):
    """a 16-packet batch of two groups of one stream configuration: one workgroup of the dense arrangement, a FIR wave per group"""
    a, b = first.batch(rolls=(0,), slack=0), second.batch(rolls=(0,))
    assert a["stream_cfgs"] == b["stream_cfgs"]
    out = dict(b)
    out["blob"] = np.concatenate([a["blob"], b["blob"]])
    out["offsets"] = np.concatenate([a["offsets"], b["offsets"] + np.uint64(a["blob"].size)])
    for k in ("sizes", "cfg_idx"):
        out[k] = np.concatenate([a[k], b[k]])
    out["slot_ints"] = max(a["slot_ints"], b["slot_ints"])
    out["status"] = a["status"] + b["status"]
    out["order"] = [(i, j) for i, j in enumerate(a["order"] + b["order"])]
    return out


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("order_class", tc.ORDER_CLASSES)
@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("kind", tc.FIR_KINDS)
def test_fir_order_class_16_packets(pkg, oracle, monkeypatch, kind, stereo, is24, order_class, arrangement):
    # narrow / wide by the variant; T = 1 / 2 / (2, L = 16) by the class; the short queue entry under the dense arrangement
    arrange(monkeypatch, arrangement)
    for block in tc.fir_blocks(kind, order_class):
        g = tc.build_fir(kind, stereo, is24, block, order_class)
        run_batch(pkg, oracle, ("16", kind, stereo, is24, order_class, block), g.batch, g.name)


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("halves", [("first_launch", "two_taps"), ("two_taps", "first_launch")])
@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("kind", ["drift", "flat_and_tie", "uniform"])
def test_fir_mixed_halves(pkg, oracle, monkeypatch, kind, stereo, is24, halves, arrangement):
    # the dense arrangement's two FIR waves run different steps (one tap, two taps) in one workgroup
    arrange(monkeypatch, arrangement)
    a, b = (tc.build_fir(kind, stereo, is24, 0, oc) for oc in halves)
    run_batch(pkg, oracle, ("halves", kind, stereo, is24, halves), lambda: two_groups(a, b), f"{a.name} + {b.name}")


def check_embedding(b):
    assert len(b["sizes"]) == tc.EMBED_PACKETS >= FOUR_TAP_MIN_PACKETS and (tc.EMBED_PACKETS + 7) // 8 > tc.L16_MAX_GROUPS
    return b


# (the first launch only hands these groups over: its 8-packet builds differ in nothing they run)
@pytest.mark.parametrize("arrangement", ["auto", "dense"])
@pytest.mark.parametrize("name,stereo,is24", EMBEDDED_CASES)
def test_entropy_case_embedded_four_taps(pkg, oracle, monkeypatch, name, stereo, is24, arrangement):
    g = tc.build(name, stereo, is24, "second_launch")
    assert max(g.ns) <= 4096
    arrange(monkeypatch, arrangement, one_range=True)
    run_batch(pkg, oracle, ("embedded", name, stereo, is24),
              lambda: check_embedding(g.embed(tc.embed_filler(stereo, is24))), f"case {name} embedded", big=True)


@pytest.mark.parametrize("arrangement", ["auto", "dense"])
@pytest.mark.parametrize("stereo,is24", tc.VARIANTS)
@pytest.mark.parametrize("kind", tc.FIR_KINDS)
def test_fir_second_launch_embedded_four_taps(pkg, oracle, monkeypatch, kind, stereo, is24, arrangement):
    arrange(monkeypatch, arrangement, one_range=True)
    g = tc.build_fir(kind, stereo, is24, 0, "second_launch")
    run_batch(pkg, oracle, ("embedded_fir", kind, stereo, is24),
              lambda: check_embedding(g.embed(tc.embed_filler(stereo, is24))), f"{g.name} embedded", big=True)
