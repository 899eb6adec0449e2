"""alacgpu_decode_window_into_device on the GPU: every packet's run starts src_skip[p] frames into the packet.  Bit-exact
against the oracle's slot output, sliced; canaries outside every run untouched; statuses equal to alacgpu_decode_into_device's;
a NULL skip array bit-identical to alacgpu_decode_into_device; a skip above 16384 is status 8 and writes nothing."""
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
    """The library's own choice of the main kernel's build, and the 16-packet arrangement, the 96-register build and the
    128-register 8-step build forced (ALACGPU_DENSE = 1 / 2 / 4, read when a context is created)."""
    value = {"dense": "1", "ab5": "2", "ab": "4"}.get(request.param)
    if value is None:
        monkeypatch.delenv("ALACGPU_DENSE", raising=False)
    else:
        monkeypatch.setenv("ALACGPU_DENSE", value)
    return request.param


def smax_of(b):
    return max(min(int(c[0]), 16384) for c in b["stream_cfgs"])


def cfg_of(b, p):
    return b["stream_cfgs"][0 if b["cfg_idx"] is None else int(b["cfg_idx"][p])]


_REF = {}


def reference(oracle, key, b):
    """The oracle's slot output (pcm, out_bytes, out_samples, status) with slot_ints = channels * Smax"""
    if key not in _REF:
        slot = int(cfg_of(b, 0)[5]) * smax_of(b)
        _REF[key] = oracle.decode_batch(oracle.make_cfgs(b["stream_cfgs"]), b["blob"], b["offsets"], b["sizes"], b["cfg_idx"],
                                        slot, n_threads=8)
    return _REF[key]


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


def run(torch, ctx, d, first, frames, skip, dtype, layout, channels, total, window=True):
    """One call into a fresh canary-filled output of total frames; skip None: a NULL skip array.  window False: the old entry
    point.  Returns (out, out_samples, status) on the host."""
    dev = torch.device("cuda", 0)
    td = torch.float32 if dtype == "float32" else torch.int32
    out = torch.full((total * channels,), CANARY_F if dtype == "float32" else CANARY_I, dtype=td, device=dev)
    os_ = torch.full((d.n,), -1, dtype=torch.int32, device=dev)
    st = torch.full((d.n,), -1, dtype=torch.int32, device=dev)
    f = torch.from_numpy(np.asarray(first, dtype=np.int64)).to(dev)
    fr = torch.from_numpy(np.asarray(frames, dtype=np.int64).astype(np.int32)).to(dev)
    ps = total if layout == "planar" else 0
    s = torch.cuda.current_stream().cuda_stream
    if window:
        sk = None if skip is None else torch.from_numpy(np.asarray(skip, dtype=np.int64).astype(np.int32)).to(dev)
        ctx.decode_window_into_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, f, fr, sk, out, channels, layout, ps, os_, st,
                                      stream=s)
    else:
        ctx.decode_into_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, f, fr, out, channels, layout, ps, os_, st, stream=s)
    torch.cuda.synchronize()
    return out.cpu().numpy(), os_.cpu().numpy(), st.cpu().numpy()


def expected(b, ref, first, frames, skip, status, dtype, layout, channels, total):
    """Canary outside the runs; in packet p's run, frame j is the oracle's frame skip[p] + j while that is decoded, else zero;
    a failed packet's run is zero (a one-channel element with status 3 keeps its residuals); status 8 writes nothing."""
    pcm, _, os_, _ = ref
    exp = np.full(total * channels, CANARY_F if dtype == "float32" else CANARY_I,
                  dtype=np.float64 if dtype == "float32" else np.int64)
    for p in range(len(first)):
        if status[p] == 8:
            continue
        n, s = int(frames[p]), int(skip[p])
        run = np.zeros((n, channels), dtype=np.int64)
        elem_mono = (int(b["blob"][int(b["offsets"][p])]) >> 5) == 0
        if status[p] == 0 or (status[p] == 3 and elem_mono):
            dec = pcm[p, :int(os_[p]) * channels].reshape(-1, channels)[s:s + n]
            run[:len(dec)] = dec
        vals = run.astype(np.float64) * 2.0 ** -(int(cfg_of(b, p)[1]) - 1) if dtype == "float32" else run
        i = np.arange(n)
        for c in range(channels):
            idx = (int(first[p]) + i) * channels + c if layout == "interleaved" else c * total + int(first[p]) + i
            exp[idx] = vals[:, c]
    return exp.astype(np.float32 if dtype == "float32" else np.int32)


def check(got, exp, what):
    if not np.array_equal(got.view(np.int32), exp.view(np.int32)):
        bad = np.nonzero(got.view(np.int32) != exp.view(np.int32))[0]
        raise AssertionError(f"{what}: {len(bad)} of {exp.size} elements differ, first at {bad[:8]}: got {got[bad[:8]]} "
                             f"want {exp[bad[:8]]}")


def random_windows(ref, seed, big_skip=()):
    """Per packet a random skip and frame count -- windows inside the decoded frames, past them (zeros), of 0 frames, at the
    packet's end, and for packets 2 and 4 the widest ones -- placed one behind the other with canary gaps; skips above 16384
    for the packets in big_skip."""
    rng = np.random.default_rng(seed)
    n_dec = np.clip(ref[2].astype(np.int64), 0, 16384)
    n = len(n_dec)
    kind = rng.integers(0, 6, n)
    skip = np.where(kind == 0, 0, (rng.random(n) * (n_dec + 1)).astype(np.int64))
    skip = np.where(kind == 1, n_dec, skip)                                   # at the end: nothing decoded is left
    skip = np.where(kind == 2, rng.integers(0, 16385, n), skip)               # anywhere up to 16384, past the decoded frames too
    room = np.maximum(n_dec - skip, 0)
    frames = np.where(kind == 3, 0, (rng.random(n) * (room + 1)).astype(np.int64))
    frames = np.where(kind == 4, room + rng.integers(1, 300, n), frames)      # longer than what is left: zeros behind
    frames = np.where(kind == 5, room, frames)                                # exactly to the packet's end
    skip[list(big_skip)] = [16385, 1 << 20, 0xFFFFFFFF][:len(big_skip)]
    # the widest windows: skip 16384 with more than 16384 frames (end 32768 and beyond: the frame count is capped at 16384 in
    # the packed window), and a window from frame 0 longer than 16384 frames
    skip[2], frames[2] = 16384, 16384 + 300
    skip[4], frames[4] = 0, 16384 + 700
    gaps = rng.integers(0, 5, n)
    first = np.cumsum(gaps) + np.concatenate([[0], np.cumsum(frames)[:-1]])
    return first, frames, skip, int(first[-1] + frames[-1]) + 3


def check_batch(torch, pkg, oracle, b, key, seed, big_skip=()):
    channels = int(cfg_of(b, 0)[5])
    ref = reference(oracle, key, b)
    first, frames, skip, total = random_windows(ref, seed, big_skip)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        for dtype, layout in COMBOS:
            out, os_, st = run(torch, ctx, d, first, frames, skip, dtype, layout, channels, total)
            _, os_old, st_old = run(torch, ctx, d, first, frames, None, dtype, layout, channels, total, window=False)
            want_st = st_old.copy()
            want_st[list(big_skip)] = 8
            assert np.array_equal(st, want_st), (dtype, layout)
            ok = np.ones(len(st), bool)
            ok[list(big_skip)] = False
            assert np.array_equal(os_[ok], os_old[ok]), (dtype, layout)
            assert np.array_equal(st[ok], ref[3][ok]), (dtype, layout)
            check(out, expected(b, ref, first, frames, skip, st, dtype, layout, channels, total), (dtype, layout))
    return ref


def test_cfg5_mixed_sizes_high_orders_escapes_and_short_packets(torch, pkg, oracle, synth):
    # cfg5: 16- and 24-bit streams in one call, LPC orders 4..31 (the second launch), escapes and short packets
    b = synth.make_config_batch(5, n_packets=192, seed=4)
    check_batch(torch, pkg, oracle, b, ("cfg5",), 1, big_skip=(5, 77, 191))


@pytest.mark.parametrize("stereo", [1, 0])
def test_ragged_mono_and_stereo_with_orders_above_8(torch, pkg, oracle, synth, stereo):
    d = synth.packet_descs(80, max_samples_per_frame=4096, stereo=stereo)
    rng = np.random.default_rng(9 + stereo)
    d["n"][rng.choice(80, 10, replace=False)] = [1, 2, 31, 33, 64, 777, 2047, 4064, 4095, 1234]
    d["pred_order"] = rng.integers(1, 17, (80, 2))
    b = synth.make_batch(d, synth.default_signal(40 + stereo))
    b.update(stream_cfgs=[(4096, 16, 40, 10, 14, 2 if stereo else 1)], cfg_idx=None)
    check_batch(torch, pkg, oracle, b, ("ragged", stereo), 2 + stereo)


def test_escapes_mono_elements_and_24bit_shift_bytes(torch, pkg, oracle, synth):
    d = synth.packet_descs(64, max_samples_per_frame=4096, n=1500)
    d["escape"][::5] = 1
    d["stereo"][1::4] = 0
    d["sample_size"][32:] = 24
    d["ub"][32::3] = 1
    d["pred_order"][:, 0] = np.arange(64) % 30 + 1
    d["pred_order"][:, 1] = (np.arange(64) * 7) % 30 + 1
    b = synth.make_batch(d, synth.default_signal(78))
    b.update(stream_cfgs=[(4096, 16, 40, 10, 14, 2), (4096, 24, 40, 10, 14, 2)], cfg_idx=(np.arange(64) >= 32).astype(np.uint16))
    ref = check_batch(torch, pkg, oracle, b, ("escapes",), 4, big_skip=(0,))
    assert (ref[3] == 0).all()


def test_failing_packets(torch, pkg, oracle, synth):
    # mutated packets: statuses as the slot layout's, failed packets' runs zero, the others' windows intact
    rng = np.random.default_rng(4321)
    src = synth.make_config_batch(5, n_packets=96, seed=97)
    blob, offs, sizes = bytearray(), [], []
    for p in range(96):
        o, s = int(src["offsets"][p]), int(src["sizes"][p])
        pkt = bytearray(bytes(src["blob"][o:o + s]))
        if p % 3 == 0:
            for _ in range(int(rng.integers(1, 6))):
                pos = int(rng.integers(3, len(pkt))) if rng.random() < 0.8 else int(rng.integers(0, min(12, len(pkt))))
                pkt[pos] ^= 1 << int(rng.integers(0, 8))
            if rng.random() < 0.2:
                pkt = pkt[: int(rng.integers(4, len(pkt)))]
        offs.append(len(blob))
        sizes.append(len(pkt))
        blob += pkt + bytes(64 * 1024)
    b = dict(src)
    b["blob"] = np.frombuffer(bytes(blob), dtype=np.uint8)
    b["offsets"] = np.array(offs, dtype=np.uint64)
    b["sizes"] = np.array(sizes, dtype=np.uint32)
    ref = check_batch(torch, pkg, oracle, b, ("mutated",), 5, big_skip=(1, 3))
    assert set(np.unique(ref[3])) - {0}, "the mutation should break at least some packets"


def test_null_skip_is_bit_identical_to_decode_into(torch, pkg, oracle, synth):
    b = synth.make_config_batch(5, n_packets=128, seed=6)
    ref = reference(oracle, ("null",), b)
    first, frames, _, total = random_windows(ref, 7)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        for dtype, layout in COMBOS:
            new = run(torch, ctx, d, first, frames, None, dtype, layout, 2, total)
            old = run(torch, ctx, d, first, frames, None, dtype, layout, 2, total, window=False)
            zero = run(torch, ctx, d, first, frames, np.zeros(d.n), dtype, layout, 2, total)
            for a, z in zip(new, old):
                assert np.array_equal(a.view(np.int32), z.view(np.int32)), (dtype, layout)
            for a, z in zip(zero, old):
                assert np.array_equal(a.view(np.int32), z.view(np.int32)), (dtype, layout)


def test_a_misaligned_skip_array_is_refused(torch, pkg, synth):
    b = synth.make_config_batch(2, n_packets=8)
    dev = torch.device("cuda", 0)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        d = Dev(torch, b)
        out = torch.zeros(2 * 8 * 4096, dtype=torch.int32, device=dev)
        first = torch.arange(8, dtype=torch.int64, device=dev) * 4096
        frames = torch.full((8,), 4096, dtype=torch.int32, device=dev)
        skip = torch.zeros(9, dtype=torch.int32, device=dev).view(torch.uint8)[1:33]
        st = torch.zeros(8, dtype=torch.int32, device=dev)
        with pytest.raises(pkg.AlacGpuError, match="rc=-"):
            ctx.decode_window_into_device(d.blob, d.nb, d.off, d.sz, d.ci, d.n, first, frames, skip, out, 2, "planar", 8 * 4096,
                                          None, st)
