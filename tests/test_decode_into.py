"""alacgpu_decode_into_device on the GPU: packets placed gap-free at dst_first in an int32 / float32 tensor, interleaved or
planar, bit-exact against the oracle (float32: exactly sample * 2^-(ss-1)); statuses equal to the slot layout's; every
element outside the runs untouched; runs of failed packets zero."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY_I = 0x5A5A5A5A
CANARY_F = 12345.5
COMBOS = [("int32", "interleaved"), ("int32", "planar"), ("float32", "interleaved"), ("float32", "planar")]


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


@pytest.fixture(autouse=True, params=["auto", "dense", "ab5", "ab"])
def arrangement(request, monkeypatch):
    """Every test runs with the library's own choice of the main kernel's build and with the 16-packet arrangement, the
    96-register build and the 128-register 8-step build forced (ALACGPU_DENSE = 1 / 2 / 4, read when a context is created)."""
    if request.param == "dense":
        monkeypatch.setenv("ALACGPU_DENSE", "1")
    elif request.param == "ab5":
        monkeypatch.setenv("ALACGPU_DENSE", "2")
    elif request.param == "ab":
        monkeypatch.setenv("ALACGPU_DENSE", "4")
    else:
        monkeypatch.delenv("ALACGPU_DENSE", raising=False)
    return request.param


_ORACLE = {}


def oracle_of(oracle, key, b, slot):
    if key not in _ORACLE:
        _ORACLE[key] = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"],
                                           slot, n_threads=8)
    return _ORACLE[key]


def smax_of(b):
    return max(min(int(c[0]), 16384) for c in b["stream_cfgs"])


def cfg_of(b, p):
    return b["stream_cfgs"][0 if b["cfg_idx"] is None else int(b["cfg_idx"][p])]


class Dev:
    """A batch resident on the device"""

    def __init__(self, torch, b):
        dev = torch.device("cuda", 0)
        nb = int(b["blob"].size)
        self.blob = torch.zeros((nb + 63) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
        self.blob[:nb] = torch.from_numpy(b["blob"]).to(dev)
        self.nb = nb
        self.off = torch.from_numpy(b["offsets"].astype(np.int64)).to(dev)
        self.sz = torch.from_numpy(b["sizes"].astype(np.int32)).to(dev)
        self.ci = None if b["cfg_idx"] is None else torch.from_numpy(b["cfg_idx"].astype(np.int16)).to(dev)
        self.n = len(b["sizes"])


def decode_into(torch, ctx, d, first, frames, dtype, layout, channels, out_elems, plane_stride=0, stream=None, out=None):
    dev = torch.device("cuda", 0)
    td = torch.float32 if dtype == "float32" else torch.int32
    if out is None:
        out = torch.full((out_elems,), CANARY_F if dtype == "float32" else CANARY_I, dtype=td, device=dev)
    os_ = torch.full((d.n,), -1, dtype=torch.int32, device=dev)
    st = torch.full((d.n,), -1, dtype=torch.int32, device=dev)
    f = torch.from_numpy(np.asarray(first, dtype=np.int64)).to(dev)
    fr = torch.from_numpy(np.asarray(frames, dtype=np.int64).astype(np.int32)).to(dev)
    s = stream if stream is not None else torch.cuda.current_stream()
    ctx.decode_into_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, f, fr, out, channels, layout, plane_stride, os_, st,
                           stream=s.cuda_stream)
    return out, os_, st, (f, fr)


def expected(b, ref, first, frames, dtype, layout, channels, out_elems, plane_stride, status=None):
    """What the destination must hold: canary outside the runs; the oracle's samples, then zeros, in every run; zero runs for
    packets that failed (a one-channel element with status 3 keeps its residuals)."""
    pcm, _, os_, st = ref
    st = st if status is None else status
    exp = np.full(out_elems, CANARY_F if dtype == "float32" else CANARY_I, dtype=np.float64 if dtype == "float32" else np.int64)
    for p in range(len(first)):
        if st[p] == 8:
            continue
        cfg = cfg_of(b, p)
        run = np.zeros((int(frames[p]), channels), dtype=np.int64)
        elem_mono = (int(b["blob"][int(b["offsets"][p])]) >> 5) == 0
        if st[p] == 0 or (st[p] == 3 and elem_mono):
            rows = min(int(os_[p]), int(frames[p]))
            run[:rows] = pcm[p, :rows * channels].reshape(rows, channels)
        vals = run.astype(np.float64) * 2.0 ** -(int(cfg[1]) - 1) if dtype == "float32" else run
        i = np.arange(int(frames[p]))
        for c in range(channels):
            idx = (int(first[p]) + i) * channels + c if layout == "interleaved" else c * plane_stride + int(first[p]) + i
            exp[idx] = vals[:, c]
    return exp.astype(np.float32 if dtype == "float32" else np.int32)


def check(torch, out, exp):
    got = out.cpu()
    want = torch.from_numpy(exp)
    if not torch.equal(got, want):
        bad = np.nonzero(got.numpy() != exp)[0]
        raise AssertionError(f"{len(bad)} of {exp.size} elements differ, first at {bad[:8]}: got {got.numpy()[bad[:8]]} "
                             f"want {exp[bad[:8]]}")


def gapless(ref, lead=7):
    """dst_first / dst_frames for the packets one behind the other (the decoded length, or 100 frames for a packet whose
    count is unusable), `lead` frames of guard in front"""
    n = ref[2].astype(np.int64)
    frames = np.where((n > 0) & (n <= 16384), n, 100)
    first = lead + np.concatenate([[0], np.cumsum(frames)[:-1]])
    return first, frames, int(first[-1] + frames[-1]) + lead


def run_all_combos(torch, pkg, oracle, b, key, first=None, frames=None, total=None, check_status=True):
    channels = int(cfg_of(b, 0)[5])
    ref = oracle_of(oracle, key, b, channels * smax_of(b))
    if first is None:
        first, frames, total = gapless(ref)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        for dtype, layout in COMBOS:
            ps = total if layout == "planar" else 0
            elems = total * channels
            out, os_, st, _ = decode_into(torch, ctx, d, first, frames, dtype, layout, channels, elems, ps)
            torch.cuda.synchronize()
            if check_status:
                assert np.array_equal(st.cpu().numpy(), ref[3]), (dtype, layout)
                assert np.array_equal(os_.cpu().numpy(), ref[2]), (dtype, layout)
            check(torch, out, expected(b, ref, first, frames, dtype, layout, channels, elems, ps, st.cpu().numpy()))
    return ref


@pytest.mark.parametrize("cfg,n", [(2, 256), (3, 40), (4, 256), (5, 320)])
def test_baseline_shapes_every_dtype_and_layout(torch, pkg, oracle, synth, cfg, n):
    # cfg5 mixes 16- and 24-bit streams in one call, LPC orders 4..31 (the second launch), escapes and short packets
    b = synth.make_config_batch(cfg, n_packets=n)
    run_all_combos(torch, pkg, oracle, b, ("cfg", cfg, n))


@pytest.mark.parametrize("stereo", [1, 0])
def test_ragged_batch_with_short_hassize_last_packets(torch, pkg, oracle, synth, stereo):
    d = synth.packet_descs(72, max_samples_per_frame=4096, stereo=stereo)
    rng = np.random.default_rng(5 + stereo)
    d["n"][rng.choice(72, 12, replace=False)] = [1, 2, 31, 32, 33, 63, 64, 65, 777, 2047, 4064, 4095]
    d["n"][-1] = 1234
    d["pred_order"] = rng.integers(1, 17, (72, 2))
    b = synth.make_batch(d, synth.default_signal(31))
    b.update(stream_cfgs=[(4096, 16, 40, 10, 14, 2 if stereo else 1)], cfg_idx=None)
    run_all_combos(torch, pkg, oracle, b, ("ragged", stereo))


def test_escapes_mono_elements_and_24bit_shift_bytes(torch, pkg, oracle, synth):
    # uncompressed packets (16 and 24 bit), one-channel elements in a two-channel stream, 24-bit with shift bytes, orders > 8
    d = synth.packet_descs(48, max_samples_per_frame=4096, n=1500)
    d["escape"][::5] = 1
    d["stereo"][1::4] = 0
    d["sample_size"][24:] = 24
    d["ub"][24::3] = 1
    d["pred_order"][:, 0] = np.arange(48) % 30 + 1
    d["pred_order"][:, 1] = (np.arange(48) * 7) % 30 + 1
    b = synth.make_batch(d, synth.default_signal(77))
    ci = (np.arange(48) >= 24).astype(np.uint16)
    b.update(stream_cfgs=[(4096, 16, 40, 10, 14, 2), (4096, 24, 40, 10, 14, 2)], cfg_idx=ci)
    ref = run_all_combos(torch, pkg, oracle, b, ("escapes",))
    assert (ref[3] == 0).all()


def test_mono_stream_with_stereo_elements(torch, pkg, oracle, synth):
    # a two-channel element in a one-channel stream comes out as its left channel (AlacFile.cs:353-354); it parks channel A
    d = synth.packet_descs(24, max_samples_per_frame=4096, n=1000, stereo=0)
    d["stereo"][::3] = 1
    b = synth.make_batch(d, synth.default_signal(8))
    b.update(stream_cfgs=[(4096, 16, 40, 10, 14, 1)], cfg_idx=None)
    ref = run_all_combos(torch, pkg, oracle, b, ("mono_stereo",))
    assert (ref[3] == 0).all()


def test_full_size_cfg2_float32_planar(torch, pkg, synth, arrangement):
    if arrangement != "auto":
        pytest.skip("one arrangement is enough at full size")
    b = synth.make_config_batch(2, want_pcm=True)          # 4096 packets x 4096 stereo frames
    T = 4096 * 4096
    first = np.arange(4096, dtype=np.int64) * 4096
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        out, os_, st, _ = decode_into(torch, ctx, d, first, np.full(4096, 4096), "float32", "planar", 2, 2 * T, T)
        torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (os_.cpu().numpy() == 4096).all()
    src = torch.from_numpy(b["pcm"].reshape(4096 * 4096, 2).T.astype(np.float32) * np.float32(2.0 ** -15)).contiguous()
    assert torch.equal(out.view(2, T).cpu(), src)


def test_statuses_of_mutated_packets_equal_the_slot_layout(torch, pkg, oracle, synth):
    # mutated packets (as test_gpu_parity.test_mutated_packets_never_hang_and_match): statuses, out_samples and the samples
    # of the packets that decode equal alacgpu_decode_batch_device's with slot_ints = C * Smax; failed packets' runs are zero
    rng = np.random.default_rng(1234)
    src = synth.make_config_batch(5, n_packets=120, seed=98)
    blob, offs, sizes = bytearray(), [], []
    for p in range(120):
        o, s = int(src["offsets"][p]), int(src["sizes"][p])
        pkt = bytearray(bytes(src["blob"][o:o + s]))
        for _ in range(int(rng.integers(1, 6))):
            pos = int(rng.integers(3, len(pkt))) if rng.random() < 0.8 else int(rng.integers(0, min(12, len(pkt))))
            pkt[pos] ^= 1 << int(rng.integers(0, 8))
        if rng.random() < 0.2:
            pkt = pkt[: int(rng.integers(4, len(pkt)))]
        offs.append(len(blob))
        sizes.append(len(pkt))
        blob += pkt + bytes(96 * 1024)
    b = dict(src)
    b["blob"] = np.frombuffer(bytes(blob), dtype=np.uint8)
    b["offsets"] = np.array(offs, dtype=np.uint64)
    b["sizes"] = np.array(sizes, dtype=np.uint32)
    slot = 2 * smax_of(b)
    dev = torch.device("cuda", 0)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        pcm = torch.zeros((d.n, slot), dtype=torch.int32, device=dev)
        ob = torch.zeros(d.n, dtype=torch.int32, device=dev)
        os_ = torch.zeros(d.n, dtype=torch.int32, device=dev)
        st = torch.zeros(d.n, dtype=torch.int32, device=dev)
        ctx.decode_batch_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, pcm, slot, ob, os_, st)
        torch.cuda.synchronize()
        slot_ref = (pcm.cpu().numpy(), ob.cpu().numpy(), os_.cpu().numpy(), st.cpu().numpy())
        assert set(np.unique(slot_ref[3])) - {0}, "the mutation should break at least some packets"
        first, frames, total = gapless(slot_ref)
        for dtype, layout in COMBOS:
            ps = total if layout == "planar" else 0
            out, os2, st2, _ = decode_into(torch, ctx, d, first, frames, dtype, layout, 2, 2 * total, ps)
            torch.cuda.synchronize()
            assert np.array_equal(st2.cpu().numpy(), slot_ref[3]) and np.array_equal(os2.cpu().numpy(), slot_ref[2])
            check(torch, out, expected(b, slot_ref, first, frames, dtype, layout, 2, 2 * total, ps))
    o = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"], slot, n_threads=8)
    assert np.array_equal(o[3], slot_ref[3])


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_canaries_truncation_and_runs_out_of_range(torch, pkg, oracle, synth, layout):
    b = synth.make_config_batch(2, n_packets=40)
    ref = oracle_of(oracle, ("cfg", 2, 40), b, 2 * 4096)
    first, frames, total = gapless(ref, lead=33)
    frames = frames.copy()
    frames[[3, 17, 39]] = [1, 4000, 0]         # shorter than the packet: truncated, out_samples still 4096
    frames[5] = 4096 + 50                      # longer: zeros behind the samples
    first = 33 + np.concatenate([[0], np.cumsum(frames)[:-1]])
    total = int(first[-1] + frames[-1]) + 40
    ps = total if layout == "planar" else 0
    elems = 2 * total
    guard = 10
    # the last two packets' runs end past out_elems (one in the guard region behind the tensor's logical end)
    first2 = first.copy()
    first2[38] = total - 5
    frames2 = frames.copy()
    frames2[38] = 100
    status = ref[3].copy()
    status[38] = 8
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        for dtype in ("int32", "float32"):
            full = torch.full((elems + guard,), CANARY_F if dtype == "float32" else CANARY_I,
                              dtype=torch.float32 if dtype == "float32" else torch.int32, device="cuda")
            out, os_, st, _ = decode_into(torch, ctx, d, first2, frames2, dtype, layout, 2, elems, ps, out=full[:elems])
            torch.cuda.synchronize()
            assert np.array_equal(st.cpu().numpy(), status)
            assert (os_.cpu().numpy() == 4096).all()
            check(torch, full[:elems], expected(b, ref, first2, frames2, dtype, layout, 2, elems, ps, status))
            assert torch.equal(full[elems:].cpu(), torch.full((guard,), CANARY_F if dtype == "float32" else CANARY_I,
                                                              dtype=full.dtype))


def test_channel_mismatch_is_status_8_and_writes_nothing(torch, pkg, oracle, synth):
    # a ctx with a stereo and a mono stream cfg: into a two-channel destination, the mono stream's packets are refused
    b = synth.make_config_batch(2, n_packets=24)
    b["cfg_idx"] = (np.arange(24) % 3 == 1).astype(np.uint16)
    b["stream_cfgs"] = [(4096, 16, 40, 10, 14, 2), (4096, 16, 40, 10, 14, 1)]
    ref = oracle_of(oracle, ("mismatch",), b, 2 * 4096)
    status = np.where(b["cfg_idx"] == 1, 8, ref[3])
    first, frames, total = gapless(ref)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        for dtype, layout in COMBOS:
            ps = total if layout == "planar" else 0
            out, os_, st, _ = decode_into(torch, ctx, d, first, frames, dtype, layout, 2, 2 * total, ps)
            torch.cuda.synchronize()
            assert np.array_equal(st.cpu().numpy(), status)
            check(torch, out, expected(b, ref, first, frames, dtype, layout, 2, 2 * total, ps, status))


def test_two_calls_in_flight_into_one_output_equal_one_call(torch, pkg, oracle, synth):
    b = synth.make_config_batch(5, n_packets=256, seed=3)
    ref = oracle_of(oracle, ("cfg5_seed3",), b, 2 * 4096)
    first, frames, total = gapless(ref)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        whole, _, st, _ = decode_into(torch, ctx, d, first, frames, "float32", "planar", 2, 2 * total, total)
        torch.cuda.synchronize()
        halves = torch.full((2 * total,), CANARY_F, dtype=torch.float32, device="cuda")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for rep in range(3):
            halves.fill_(CANARY_F)
            torch.cuda.synchronize()
            keep = []
            for (lo, hi), s in (((0, 128), s1), ((128, 256), s2)):
                h = Dev.__new__(Dev)
                h.blob, h.nb, h.n = d.blob, d.nb, hi - lo
                h.off, h.sz, h.ci = d.off[lo:hi], d.sz[lo:hi], d.ci[lo:hi]
                with torch.cuda.stream(s):
                    keep.append(decode_into(torch, ctx, h, first[lo:hi], frames[lo:hi], "float32", "planar", 2, 2 * total, total,
                                            stream=s, out=halves))
            torch.cuda.synchronize()
            assert torch.equal(halves, whole), rep
            assert np.array_equal(np.concatenate([k[2].cpu().numpy() for k in keep]), st.cpu().numpy())
