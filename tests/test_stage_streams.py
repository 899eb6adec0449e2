"""When and where the stage calls run: the stream of every launch, and the scratch protocol of alacgpu_ctx.h between calls
of one context on different streams.  The other test files check what the kernels compute, all on the default stream.

Every case keeps a side stream busy with a gate (stage_stream_calls.Gate: a delay of GATE_MS behind which an event is
recorded) and enqueues its calls while the gate is pending.  Each case measures the host time of its enqueues with
time.perf_counter, prints it next to the gate's own duration from its timing events, and asserts that the gate was still pending
when the enqueues had returned: a host too slow for the delay fails the case, it cannot pass it unchecked.
Measured on an MI355X (torch.cuda._sleep as the delay, 2.4 million of its cycles per millisecond): the enqueues of a case take
0.05 to 0.9 ms of host time, those of the first case of a process, whose kernels are loaded then, 6.0 ms.  GATE_MS = 60 is ten
times the longest of them and seventy times the usual one; the gates themselves took 59.8 to 60.8 ms.

Part 1, test_every_launch_runs_on_its_stream: per entry point, the inputs are poison and the output a sentinel until, behind
the gate and on the same side stream, the true inputs are copied in; then the call; then a clone of the output.  A launch on
the null stream reads poison (it does not wait for the gate), a last launch on another stream leaves the sentinel in the clone.
Part 2, the scratch protocol per family (enc, scan, norm, mix, reverb): the wait of a second stream, a 0-byte call in between,
the host's wait before the scratch grows, 32 rounds back to back, close() behind pending work, reverb's first call.
The encoder's calls are test_encode_policy.run's -- its tensors, canary and argument order -- made here without the
synchronise that `run` has in front of its call (it would wait for the gate); `run` itself gives the packets A's reference is
compared with, and its `unpack` reads them.
Part 3: the public functions, which share one context per device, from two streams.  `resample` and `speed_perturb` upload
their lengths and tables inside the call, which holds the host until the gate has passed: they are compared, not event-tested.

Every comparison is bit for bit with the same call made alone on the default stream of a fresh context (Part 3: through the
same public function alone on the default stream)."""
import time

import pytest

import stage_stream_calls as sc
from stage_stream_calls import CFG, Gate, alone, same_bits, too_short

pytestmark = pytest.mark.gpu

GATE_MS = 60.0
ROWS_A = 64              # Part 2: A's rows, so that A and B differ in grid size


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.device_count() > 0
    t.cuda.set_device(0)
    sc.calibrate(t)          # (the gate's unit, measured outside every case's own timing)
    return t


@pytest.fixture(scope="module")
def pkg():
    import alac.net_amd as p

    p.lib()
    return p


def align_up(v, a):
    return (v + a - 1) // a * a


def allocated(need):
    """What scratch::acquire allocates for a need that does not fit: 25 % slack, rounded up to 4096 bytes"""
    return align_up(need + need // 4, 4096)


# ---- Part 1 ----------------------------------------------------------------------------------------------------------------------
def entries(torch, pkg):
    tile = sc.scan_tile()
    wave, lds = sc.header_constant("ALAC_NORM_WAVE_MAX", "alac_normalize.h"), sc.header_constant("ALAC_NORM_LDS_MAX", "alac_normalize.h")
    top, mix = sc.header_constant("ALAC_TOP_PART", "alac_normalize.h"), sc.header_constant("ALAC_MIX_PART", "alac_mix.h")
    return {
        "plan_crops": lambda: sc.plan_call(torch, pkg, False),
        "plan_crops_frames": lambda: sc.plan_call(torch, pkg, True),
        "compact_packets-1": lambda: sc.compact_call(torch, pkg, tile),
        "compact_packets-2": lambda: sc.compact_call(torch, pkg, tile + 1),
        "compact_packets-3": lambda: sc.compact_call(torch, pkg, tile * tile + 1),
        "stage_packets-1": lambda: sc.stage_call(torch, pkg, tile),
        "stage_packets-2": lambda: sc.stage_call(torch, pkg, tile + 1),
        "stage_packets-3": lambda: sc.stage_call(torch, pkg, tile * tile + 1),
        "resample": lambda: sc.resample_call(torch, pkg),
        "resample_rows": lambda: sc.resample_rows_call(torch, pkg),
        "resample_ratio_rows": lambda: sc.resample_ratio_rows_call(torch, pkg),
        "logmel": lambda: sc.transform_call(torch, pkg, pkg.LogMel(16000, n_fft=400, hop_length=160, n_mels=20), 20),
        "fbank": lambda: sc.transform_call(torch, pkg, pkg.KaldiFbank(16000, n_mels=23), 23),
        "mfcc": lambda: sc.transform_call(torch, pkg, pkg.KaldiMfcc(16000), 13),
        "deltas": lambda: sc.deltas_call(torch, pkg),
        "normalize_meanvar-wave": lambda: sc.meanvar_call(torch, pkg, wave - 3),
        "normalize_meanvar-lds": lambda: sc.meanvar_call(torch, pkg, wave + 1),
        "normalize_meanvar-memory": lambda: sc.meanvar_call(torch, pkg, lds + 1),
        "normalize_top-1": lambda: sc.top_call(torch, pkg, 300),
        "normalize_top-2": lambda: sc.top_call(torch, pkg, top + 1),
        "specaugment": lambda: sc.specaugment_call(torch, pkg),
        "mix-1": lambda: sc.mix_call(torch, pkg, 300),
        "mix-2": lambda: sc.mix_call(torch, pkg, mix + 1),
        "reverb": lambda: sc.reverb_call(torch, pkg),
    }


ENTRIES = ["plan_crops", "plan_crops_frames", "compact_packets-1", "compact_packets-2", "compact_packets-3", "stage_packets-1",
           "stage_packets-2", "stage_packets-3", "resample", "resample_rows", "resample_ratio_rows", "logmel", "fbank", "mfcc", "deltas",
           "normalize_meanvar-wave", "normalize_meanvar-lds", "normalize_meanvar-memory", "normalize_top-1", "normalize_top-2",
           "specaugment", "mix-1", "mix-2", "reverb"]


def behind_a_gate(torch, pkg, call, what):
    """Part 1's steps for one call on a fresh context; returns the clone of its outputs"""
    s = torch.cuda.Stream()
    call.poison()
    torch.cuda.synchronize()
    with pkg.AlacGpuContext(CFG) as ctx:
        t0 = time.perf_counter()
        gate = Gate(torch, s, GATE_MS)
        with torch.cuda.stream(s):
            call.load()
        call.run(ctx, s.cuda_stream)
        with torch.cuda.stream(s):
            got = call.clones()
        spent = time.perf_counter() - t0
        pending = gate.pending()
        torch.cuda.synchronize()
    print(f"[enqueue] {what}: {spent * 1e3:.3f} ms of host time")
    gate.report(what)
    assert pending, too_short(what, GATE_MS, spent)
    return got


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_launch_runs_on_its_stream(torch, pkg, entry):
    table = entries(torch, pkg)
    assert sorted(table) == sorted(ENTRIES)
    call = table[entry]()
    want = alone(torch, pkg, call)
    got = behind_a_gate(torch, pkg, call, entry)
    assert same_bits(torch, got, want), f"{entry}: behind a gate on a side stream the call gives other bits than alone on the default stream"


# ---- Part 2 ----------------------------------------------------------------------------------------------------------------------
class Family:
    """A family's calls: a(seed) with ROWS_A rows' worth of work, b(seed) with less and other inputs, big(seed) whose need
    is at least 2.5 times a's and more than a's call allocates (checked where the family is defined), z(seed) that needs no
    scratch (scan only)."""

    def __init__(self, a, b, big, z=None):
        self.a, self.b, self.big, self.z = a, b, big, z


def families(torch, pkg):
    tile = sc.scan_tile()
    top, mix = sc.header_constant("ALAC_TOP_PART", "alac_normalize.h") + 1, sc.header_constant("ALAC_MIX_PART", "alac_mix.h") + 1
    n_a, n_big = ROWS_A * tile + 1, tile * tile + 1
    assert 0 < sc.scan_need(tile + 1) <= sc.scan_need(n_a) and sc.scan_need(tile) == 0
    assert sc.scan_need(n_big) >= 2.5 * sc.scan_need(n_a) and sc.scan_need(n_big) > allocated(sc.scan_need(n_a))
    top_big = 700
    assert sc.top_need(top_big, top) >= 2.5 * sc.top_need(ROWS_A, top) and sc.top_need(top_big, top) > allocated(sc.top_need(ROWS_A, top))
    mix_big = 350
    assert sc.mix_need(mix_big, mix) >= 2.5 * sc.mix_need(ROWS_A, mix) and sc.mix_need(mix_big, mix) > allocated(sc.mix_need(ROWS_A, mix))
    reverb_big = 3 * ROWS_A
    assert sc.reverb_spectra(reverb_big) >= 2.5 * (sc.reverb_spectra(ROWS_A) + 64 * ROWS_A)
    assert sc.reverb_spectra(reverb_big) > allocated(sc.reverb_spectra(ROWS_A) + 64 * ROWS_A)
    enc_big = 3 * ROWS_A                                         # (the encoder's workspace is one packet's times the packets of a round)
    assert enc_big <= torch.cuda.get_device_properties(0).multi_processor_count * 16
    return {
        "enc": Family(lambda s: sc.encode_call(torch, pkg, ROWS_A, s), lambda s: sc.encode_call(torch, pkg, 7, s),
                      lambda s: sc.encode_call(torch, pkg, enc_big, s)),
        "scan": Family(lambda s: sc.compact_call(torch, pkg, n_a, s), lambda s: sc.stage_call(torch, pkg, tile + 1, s),
                       lambda s: sc.compact_call(torch, pkg, n_big, s), lambda s: sc.compact_call(torch, pkg, tile, s)),
        "norm": Family(lambda s: sc.top_call(torch, pkg, top, s, ROWS_A), lambda s: sc.top_call(torch, pkg, top, s, 3),
                       lambda s: sc.top_call(torch, pkg, top, s, top_big)),
        "mix": Family(lambda s: sc.mix_call(torch, pkg, mix, s, ROWS_A), lambda s: sc.mix_call(torch, pkg, mix, s, 3),
                      lambda s: sc.mix_call(torch, pkg, mix, s, mix_big)),
        "reverb": Family(lambda s: sc.reverb_call(torch, pkg, s, ROWS_A), lambda s: sc.reverb_call(torch, pkg, s, 3),
                         lambda s: sc.reverb_call(torch, pkg, s, reverb_big)),
    }


FAMILIES = ["enc", "scan", "norm", "mix", "reverb"]


def ready(torch, *calls):
    """The calls' inputs in place and their outputs sentinels, behind a full synchronise"""
    for c in calls:
        c.poison()
        c.load()
    torch.cuda.synchronize()


def record(torch, stream):
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def finishes_behind(evA, evB, what):
    """B's stream can have passed evB only behind A: the event test of the wait"""
    evB.synchronize()
    assert evA.query(), f"{what}: B had finished while A was still pending: its stream did not wait for the scratch's last user"


@pytest.mark.parametrize("family", FAMILIES)
def test_the_second_stream_waits(torch, pkg, family):
    f = families(torch, pkg)[family]
    A, B = f.a(1), f.b(2)
    wantA, wantB = alone(torch, pkg, A), alone(torch, pkg, B)
    if family == "enc":      # and the reference is what test_encode_policy's `run` gives for the same packets
        pk, st = A.policy()[:2]
        got = A.unpack(wantA)
        assert (st == 0).all() and (got[1] == 0).all() and got[0] == pk
    ready(torch, A, B)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext(CFG) as ctx:
        t0 = time.perf_counter()
        gate = Gate(torch, s1, GATE_MS)
        A.run(ctx, s1.cuda_stream)
        evA = record(torch, s1)
        B.run(ctx, s2.cuda_stream)
        evB = record(torch, s2)
        spent = time.perf_counter() - t0
        assert not evA.query(), too_short(family, GATE_MS, spent)
        finishes_behind(evA, evB, family)
        torch.cuda.synchronize()
    print(f"[enqueue] wait {family}: {spent * 1e3:.3f} ms of host time")
    gate.report(f"wait {family}")
    assert same_bits(torch, A.outs, wantA) and same_bits(torch, B.outs, wantB)


def test_a_call_without_scratch_between_two_with(torch, pkg):
    """A pending on s1, Z (one scan tile: 0 bytes) on s2, B on s3: Z is right while A is pending -- it reads and writes
    nothing of the buffer A owns -- and B still finishes behind A: Z has not replaced A's event"""
    f = families(torch, pkg)["scan"]
    A, Z, B = f.a(1), f.z(3), f.b(2)
    wantA, wantZ, wantB = alone(torch, pkg, A), alone(torch, pkg, Z), alone(torch, pkg, B)
    ready(torch, A, Z, B)
    # Z is read back on its own stream into page-locked memory: work on the default stream in this window can share a hardware
    # queue with the gated stream and then waits for the gate
    hostZ, wantZ_host = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in Z.outs], [w.cpu() for w in wantZ]
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext(CFG) as ctx:
        t0 = time.perf_counter()
        gate = Gate(torch, s1, GATE_MS)
        A.run(ctx, s1.cuda_stream)
        evA = record(torch, s1)
        Z.run(ctx, s2.cuda_stream)
        with torch.cuda.stream(s2):
            for h, o in zip(hostZ, Z.outs):
                h.copy_(o, non_blocking=True)
        s2.synchronize()
        z_right = same_bits(torch, hostZ, wantZ_host)
        B.run(ctx, s3.cuda_stream)
        evB = record(torch, s3)
        spent = time.perf_counter() - t0
        assert not evA.query(), too_short("scan with a 0-byte call", GATE_MS, spent)
        assert z_right, "the 0-byte call is wrong while the scratch's owner is pending"
        finishes_behind(evA, evB, "scan behind a 0-byte call")
        torch.cuda.synchronize()
    print(f"[enqueue] 0-byte call: {spent * 1e3:.3f} ms of host time (Z's result is compared inside it)")
    gate.report("0-byte call")
    assert same_bits(torch, A.outs, wantA) and same_bits(torch, B.outs, wantB) and same_bits(torch, Z.outs, wantZ)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_host_waits_before_the_scratch_grows(torch, pkg, family):
    f = families(torch, pkg)[family]
    A1, A2, B1, B2 = f.a(1), f.a(1), f.big(2), f.big(2)
    wantA, wantB = alone(torch, pkg, A1), alone(torch, pkg, B1)
    ready(torch, A1, A2, B1, B2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext(CFG) as ctx:
        t0 = time.perf_counter()
        gate = Gate(torch, s1, GATE_MS)
        A1.run(ctx, s1.cuda_stream)
        evA = record(torch, s1)
        spent = time.perf_counter() - t0
        assert not evA.query(), too_short(family, GATE_MS, spent)
        B1.run(ctx, s2.cuda_stream)
        assert evA.query(), f"{family}: the call that grows the scratch returned while its last user was pending"
        A2.run(ctx, s1.cuda_stream)
        B2.run(ctx, s2.cuda_stream)
        torch.cuda.synchronize()
    print(f"[enqueue] grow {family}: {spent * 1e3:.3f} ms of host time")
    gate.report(f"grow {family}")
    for got, want, name in ((A1, wantA, "A"), (B1, wantB, "B"), (A2, wantA, "A again"), (B2, wantB, "B again")):
        assert same_bits(torch, got.outs, want), (family, name)


@pytest.mark.parametrize("family", FAMILIES)
def test_back_to_back_on_two_streams(torch, pkg, family):
    """A on s1, B on s2, A on s1 for 32 rounds -- more than there are launch slots -- with no gate and no host wait; each
    call's outputs are cloned on its stream behind it"""
    f = families(torch, pkg)[family]
    A, B = f.a(1), f.b(2)
    wantA, wantB = alone(torch, pkg, A), alone(torch, pkg, B)
    ready(torch, A, B)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = []
    with pkg.AlacGpuContext(CFG) as ctx:
        for _ in range(32):
            for call, s, want in ((A, s1, wantA), (B, s2, wantB), (A, s1, wantA)):
                call.run(ctx, s.cuda_stream)
                with torch.cuda.stream(s):
                    got.append((call.clones(), want))
        torch.cuda.synchronize()
    wrong = [k for k, (g, want) in enumerate(got) if not same_bits(torch, g, want)]
    assert not wrong, f"{family}: calls {wrong} of {len(got)} (A, B, A per round) differ from the call made alone"


@pytest.mark.parametrize("family", FAMILIES)
def test_close_waits_for_the_last_user(torch, pkg, family):
    A = families(torch, pkg)[family].a(1)
    wantA = alone(torch, pkg, A)
    ready(torch, A)
    s1 = torch.cuda.Stream()
    ctx = pkg.AlacGpuContext(CFG)
    try:
        t0 = time.perf_counter()
        gate = Gate(torch, s1, GATE_MS)
        A.run(ctx, s1.cuda_stream)
        evA = record(torch, s1)
        spent = time.perf_counter() - t0
        assert not evA.query(), too_short(family, GATE_MS, spent)
        ctx.close()
        assert evA.query(), f"{family}: close() returned while the scratch's last user was pending"
    finally:
        torch.cuda.synchronize()
        ctx.close()
    print(f"[enqueue] close {family}: {spent * 1e3:.3f} ms of host time")
    gate.report(f"close {family}")
    assert same_bits(torch, A.outs, wantA)


def test_reverbs_first_call_on_a_side_stream(torch, pkg):
    """The context's twiddle table is made by its first reverb call: behind a gate on a side stream here, ROWS_A rows"""
    A = sc.reverb_call(torch, pkg, 5, ROWS_A)
    want = alone(torch, pkg, A)
    assert same_bits(torch, behind_a_gate(torch, pkg, A, "reverb's first call"), want)


# ---- Part 3 ----------------------------------------------------------------------------------------------------------------------
def public_calls(torch, pkg):
    """name -> (the call on inputs made from a seed, whether it uses the context's scratch).  Nothing here uploads from the
    host inside the call where the event test needs the call to return at once."""
    top, mix = sc.header_constant("ALAC_TOP_PART", "alac_normalize.h") + 1, sc.header_constant("ALAC_MIX_PART", "alac_mix.h") + 1
    f = sc.reverb_frames()
    randn = lambda shape, seed: sc._randn(torch, shape, 2000 + seed)
    rows = lambda seed: 8 if seed == 1 else 3                    # (the gated call is the larger: the other needs no more scratch)
    decay = torch.exp(-torch.arange(f, device="cuda", dtype=torch.float32) / 300.0)
    logmel, fbank, mfcc = pkg.LogMel(16000, n_fft=400, hop_length=160, n_mels=20), pkg.KaldiFbank(16000, n_mels=23), pkg.KaldiMfcc(16000)
    draws = (torch.tensor([[150, 153], [100, 96]], dtype=torch.int32, device="cuda"),
             torch.tensor([[[1, 2]], [[5, 3]]], dtype=torch.int32, device="cuda"),
             torch.tensor([[[10, 20]], [[200, 50]]], dtype=torch.int32, device="cuda"))

    def prepared(make, call):
        def build(seed):
            args = make(seed)
            return lambda: call(*args)
        return build

    return {
        "reverb": (prepared(lambda s: (randn((rows(s), 1, f), s), randn((rows(s), 1, f), 50 + s) * decay), lambda x, h: [pkg.reverb(x, h)]), True),
        "mix": (prepared(lambda s: (randn((rows(s), 2, mix), s), randn((rows(s), 1, mix), 50 + s), torch.full((rows(s),), 10.0 + s, device="cuda")),
                         lambda x, n, snr: [pkg.mix(x, n, snr)]), True),
        "normalize": (prepared(lambda s: (randn((rows(s), 1, top), s),), lambda x: [pkg.normalize(x, pkg.TopDb(1.5, 0.25, 1.0))]), True),
        "spec_augment": (prepared(lambda s: (randn((2, 1, 8, 300), s),), lambda x: [pkg.spec_augment(x, draws)]), False),
        "resample": (prepared(lambda s: (randn((2, 2, 3000), s),), lambda x: list(pkg.resample(x, 44100, 16000, lengths=[3000, 2500]))), False),
        "speed_perturb": (prepared(lambda s: (randn((2, 2, 3000), s),), lambda x: list(pkg.speed_perturb(x, [0.9, 1.0], 16000))), False),
        "log_mel": (prepared(lambda s: (0.1 * randn((2, 2000), s),), lambda x: [pkg.log_mel(x, logmel)]), False),
        "fbank": (prepared(lambda s: (0.1 * randn((2, 2000), s),), lambda x: [pkg.fbank(x, fbank)]), False),
        "mfcc": (prepared(lambda s: (0.1 * randn((2, 2000), s),), lambda x: [pkg.mfcc(x, mfcc)]), False),
    }


PUBLIC = ["reverb", "mix", "normalize", "spec_augment", "resample", "speed_perturb", "log_mel", "fbank", "mfcc"]


@pytest.mark.parametrize("name", PUBLIC)
def test_public_functions_from_two_streams(torch, pkg, name):
    table = public_calls(torch, pkg)
    assert sorted(table) == sorted(PUBLIC)
    build, uses_scratch = table[name]
    callA, callB = build(1), build(2)
    wantA, wantB = callA(), callB()                              # alone on the default stream (and the shared context is warm)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t0 = time.perf_counter()
    gate = Gate(torch, s1, GATE_MS)
    with torch.cuda.stream(s1):
        gotA = callA()
        evA = record(torch, s1)
    with torch.cuda.stream(s2):
        gotB = callB()
        evB = record(torch, s2)
    spent = time.perf_counter() - t0
    if uses_scratch:
        assert not evA.query(), too_short(name, GATE_MS, spent)
        finishes_behind(evA, evB, name)
    torch.cuda.synchronize()
    print(f"[enqueue] public {name}: {spent * 1e3:.3f} ms of host time")
    gate.report(f"public {name}")
    assert same_bits(torch, gotA, wantA), f"{name}: the call behind a gate on a side stream differs from the call alone"
    assert same_bits(torch, gotB, wantB), f"{name}: the call on the second stream differs from the call alone"
