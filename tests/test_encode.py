"""alacgpu_encode_device and alac.net_amd.save / save_batch on the GPU: every packet byte-exact against the CPU encoder run on
the recipe read back from its header; decode(encode(pcm)) == pcm through the C oracle and the GPU decoder; the size policy;
M4A files through load, packet_table and AlacContext; statuses with untouched slots."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5


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


def encode(torch, pkg, planar, stream_cfgs, firsts, frames, cfg_idx=None, dtype=None, slot=None, packets=None):
    """planar [C, T] numpy int32 (or a device tensor); returns (packet bytes list, status, raw slot buffer, slot)."""
    C_ = planar.shape[0]
    pcm = planar if isinstance(planar, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(planar, dtype=np.int32))
    if dtype == torch.float32 and pcm.dtype != torch.float32:
        ss = stream_cfgs[0][1]
        pcm = pcm.to(torch.float32) * 2.0 ** -(ss - 1)
    pcm = pcm.cuda()
    n = len(frames)
    ci = np.zeros(n, np.uint16) if cfg_idx is None else np.asarray(cfg_idx, np.uint16)
    if slot is None:
        slot = max(pkg.encode_max_packet_bytes(min(c[0], 16384), c[1], C_) for c in stream_cfgs)
    d_packets = torch.full((n * slot,), CANARY, dtype=torch.uint8, device="cuda") if packets is None else packets
    d_sizes = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    with pkg.AlacGpuContext(stream_cfgs) as ctx:
        ctx.encode_device(pcm, C_, torch.from_numpy(np.asarray(firsts, np.int64)).cuda(),
                          torch.from_numpy(np.asarray(frames, np.int32)).cuda(), torch.from_numpy(ci.astype(np.int16)).cuda(), n,
                          d_packets, slot, d_sizes, d_st, layout="planar", plane_stride=pcm.shape[1],
                          stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    raw = d_packets.cpu().numpy()
    sizes, st = d_sizes.cpu().numpy(), d_st.cpu().numpy()
    pk = [raw[p * slot:p * slot + int(sizes[p])].tobytes() for p in range(n)]
    return pk, st, raw, slot, sizes


def split(T, frame_len):
    firsts = np.arange(0, T, frame_len, dtype=np.int64)
    return firsts, np.minimum(T - firsts, frame_len)


class Bits:
    def __init__(self, data):
        self.v, self.n, self.pos = int.from_bytes(data, "big"), len(data) * 8, 0

    def read(self, k):
        self.pos += k
        return (self.v >> (self.n - self.pos)) & ((1 << k) - 1) if k else 0


def recipe(synth, pkt, cfg):
    """The synth recipe (coef_mode 1) a GPU packet's header spells out."""
    max_spf, ss, pb, mb, kb, nc = cfg
    b = Bits(pkt)
    chfield = b.read(3)
    b.read(16)
    hassize, ub, esc = b.read(1), b.read(2), b.read(1)
    n = b.read(32) if hassize else max_spf
    stereo = chfield == 1
    assert chfield == (1 if nc == 2 else 0)
    d = synth.packet_descs(1, n=n, max_samples_per_frame=max_spf, sample_size=ss, stereo=int(stereo), ub=ub, escape=esc,
                           coef_mode=1, rice_history_mult=pb, rice_initial_history=mb, rice_kmodifier=kb)
    if not esc:
        d["mix_shift"], d["mix_weight"] = b.read(8), b.read(8)
        for c in range(2 if stereo else 1):
            d["pred_type"][0, c], d["quant"][0, c], d["ricemod"][0, c], d["pred_order"][0, c] = b.read(4), b.read(4), b.read(3), b.read(5)
            for j in range(int(d["pred_order"][0, c])):
                v = b.read(16)
                d["coefs"][0, c, j] = v - 65536 if v > 32767 else v
    return d, bool(hassize), n


def check_twin(synth, packets, planar, firsts, frames, cfgs, cfg_idx=None):
    """Every packet equals the CPU encoder's on its recipe; returns the recipes."""
    out = []
    for p, pkt in enumerate(packets):
        cfg = cfgs[0 if cfg_idx is None else int(cfg_idx[p])]
        d, hassize, n = recipe(synth, pkt, cfg)
        assert n == frames[p] and hassize == (frames[p] != cfg[0]), p
        src = planar[:, firsts[p]:firsts[p] + frames[p]].T.reshape(-1)
        assert synth.encode_packet(d, src) == pkt, f"packet {p} differs from the CPU encoder"
        out.append(d)
    return out


def source(synth, C_, ss, n_packets, frame_len, last, seed=7):
    sig = synth.default_signal(seed)
    parts = [synth.make_pcm(sig, p, ss, C_, frame_len if p < n_packets - 1 else last).reshape(-1, C_) for p in range(n_packets)]
    return np.ascontiguousarray(np.concatenate(parts).T)


@pytest.mark.parametrize("ss,C_", [(16, 2), (24, 2), (16, 1), (24, 1)])
@pytest.mark.parametrize("n_packets", [1, 7])
def test_byte_exact_against_cpu_encoder(torch, pkg, synth, ss, C_, n_packets):
    last = 1234 if n_packets > 1 else 4096
    planar = source(synth, C_, ss, n_packets, 4096, last)
    cfgs = [(4096, ss, 40, 10, 14, C_)]
    firsts, frames = split(planar.shape[1], 4096)
    pk, st, _, slot, _ = encode(torch, pkg, planar, cfgs, firsts, frames)
    assert (st == 0).all()
    ds = check_twin(synth, pk, planar, firsts, frames, cfgs)
    for d in ds:   # the fixed policy: 24-bit packets carry one low byte (mono too), 16-bit none; escape packets none
        if not d["escape"][0]:
            assert int(d["ub"][0]) == (1 if ss == 24 else 0)
            assert list(d["pred_order"][0, :C_]) == [8] * C_ and list(d["quant"][0, :C_]) == [9] * C_
            assert list(d["ricemod"][0, :C_]) == [4] * C_ and list(d["pred_type"][0, :C_]) == [0] * C_
            if C_ == 2:
                assert int(d["mix_shift"][0]) == 2 and 0 <= int(d["mix_weight"][0]) <= 4
    assert all(len(x) <= slot for x in pk)


def test_byte_exact_4096_packets_cfg2(torch, pkg, synth):
    planar = source(synth, 2, 16, 4096, 4096, 4096, seed=11)
    cfgs = [(4096, 16, 40, 10, 14, 2)]
    firsts, frames = split(planar.shape[1], 4096)
    pk, st, _, _, _ = encode(torch, pkg, planar, cfgs, firsts, frames)
    assert (st == 0).all()
    check_twin(synth, pk, planar, firsts, frames, cfgs)


def roundtrip(torch, pkg, oracle, planar, cfgs, firsts, frames, cfg_idx=None, dtype=None):
    """Encodes, then decodes through the C oracle and through decode_into_device; both must give planar back."""
    C_ = planar.shape[0]
    pk, st, _, slot, sizes = encode(torch, pkg, planar, cfgs, firsts, frames, cfg_idx, dtype)
    assert (st == 0).all(), st
    n = len(pk)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum([((len(x) + 15) // 16) * 16 for x in pk])[:-1]
    blob = np.zeros(int(offs[-1]) + len(pk[-1]) + 64, np.uint8)
    for o, x in zip(offs, pk):
        blob[int(o):int(o) + len(x)] = np.frombuffer(x, np.uint8)
    sz = np.array([len(x) for x in pk], np.uint32)
    smax = max(min(c[0], 16384) for c in cfgs)
    ref, _, osm, rst = oracle.decode_batch(oracle.make_cfgs(cfgs), blob, offs, sz, cfg_idx, smax * C_, n_threads=8)
    assert (rst == 0).all() and (osm == np.asarray(frames)).all()
    for p in range(n):
        assert np.array_equal(ref[p, :frames[p] * C_].reshape(-1, C_).T, planar[:, firsts[p]:firsts[p] + frames[p]]), p
    T = planar.shape[1]
    out = torch.full((C_, T), -99, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    ci = torch.from_numpy((np.zeros(n) if cfg_idx is None else np.asarray(cfg_idx)).astype(np.int16)).cuda()
    with pkg.AlacGpuContext(cfgs) as ctx:
        ctx.decode_into_device(torch.from_numpy(blob).cuda(), len(blob) - 64, torch.from_numpy(offs.astype(np.int64)).cuda(),
                               torch.from_numpy(sz.astype(np.int32)).cuda(), ci, n, torch.from_numpy(firsts.astype(np.int64)).cuda(),
                               torch.from_numpy(np.asarray(frames, np.int32)).cuda(), out, C_, "planar", T, None, d_st,
                               stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all()
    assert np.array_equal(out.cpu().numpy(), planar)
    return pk, sizes


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_round_trip_config_shaped(torch, pkg, synth, oracle, cfg):
    d, sig, stream_cfgs, cfg_idx = synth.config_descs(cfg, n_packets=24)
    C_ = int(stream_cfgs[0][5])
    frames = d["n"].astype(np.int64)
    firsts = np.concatenate([[0], np.cumsum(frames)[:-1]])
    parts = []
    for p in range(len(d)):
        ss = stream_cfgs[0 if cfg_idx is None else int(cfg_idx[p])][1]
        parts.append(synth.make_pcm(sig, p, ss, C_, int(frames[p])).reshape(-1, C_))
    planar = np.ascontiguousarray(np.concatenate(parts).T)
    roundtrip(torch, pkg, oracle, planar, stream_cfgs, firsts, frames, cfg_idx)
    if cfg in (2, 3):
        roundtrip(torch, pkg, oracle, planar, stream_cfgs, firsts, frames, cfg_idx, dtype=torch.float32)


@pytest.mark.parametrize("ss,C_", [(16, 2), (24, 2), (16, 1), (24, 1)])
def test_round_trip_adversarial(torch, pkg, synth, oracle, ss, C_):
    lo, hi = -(1 << (ss - 1)), (1 << (ss - 1)) - 1
    cfgs = [(4096, ss, 40, 10, 14, C_)]
    T = 4096 * 3 + 100
    firsts, frames = split(T, 4096)
    # digital silence, one packet wholly silent: the zero-run mode
    silent = np.zeros((C_, T), np.int32)
    silent[:, 4096 * 2 + 10:] = 5
    pk, _ = roundtrip(torch, pkg, oracle, silent, cfgs, firsts, frames)
    check_twin(synth, pk, silent, firsts, frames, cfgs)
    # alternating full-scale extremes: the residual wraps at rss bits
    alt = np.where(np.arange(T) % 2 == 0, lo, hi).astype(np.int32)[None].repeat(C_, 0)
    if C_ == 2:
        alt[1] = alt[1, ::-1]
    pk, _ = roundtrip(torch, pkg, oracle, np.ascontiguousarray(alt), cfgs, firsts, frames)
    check_twin(synth, pk, alt, firsts, frames, cfgs)
    # full-scale white noise: escape packets
    noise = np.random.default_rng(ss + C_).integers(lo, hi + 1, (C_, T)).astype(np.int32)
    pk, sizes = roundtrip(torch, pkg, oracle, noise, cfgs, firsts, frames)
    ds = check_twin(synth, pk, noise, firsts, frames, cfgs)
    assert all(int(d["escape"][0]) == 1 for d in ds)
    # one-frame packets
    T1 = 9
    f1, n1 = np.arange(T1, dtype=np.int64), np.ones(T1, np.int64)
    one = np.random.default_rng(3).integers(lo, hi + 1, (C_, T1)).astype(np.int32)
    pk, _ = roundtrip(torch, pkg, oracle, one, cfgs, f1, n1)
    check_twin(synth, pk, one, f1, n1, cfgs)


def test_size_policy_against_cpu_encoder(torch, pkg, synth):
    n = 512
    d = synth.packet_descs(n)                               # weight 1, order 8, q 9, coef_mode 0: LPC on the packet
    b = synth.make_batch(d, synth.default_signal(0xA1AC0000 + (2 << 24)), want_pcm=True)
    planar = np.ascontiguousarray(b["pcm"].reshape(-1, 2).T)
    firsts, frames = split(planar.shape[1], 4096)
    pk, st, _, slot, _ = encode(torch, pkg, planar, [(4096, 16, 40, 10, 14, 2)], firsts, frames)
    assert (st == 0).all()
    gpu, cpu = sum(len(x) for x in pk), int(b["sizes"].sum())
    assert gpu <= 1.002 * cpu, (gpu, cpu)
    assert max(len(x) for x in pk) <= pkg.encode_max_packet_bytes(4096, 16, 2) == slot


def test_statuses_and_untouched_slots(torch, pkg):
    T = 5000
    planar = (np.arange(2 * T, dtype=np.int32).reshape(2, T) % 300) - 150
    cfgs = [(1024, 16, 40, 10, 14, 2)]
    firsts = np.array([0, 100, 4990, 1024, 200, 0], np.int64)
    frames = np.array([1024, 0, 11, 1025, 500, 1], np.int64)
    pk, st, raw, slot, sizes = encode(torch, pkg, planar, cfgs, firsts, frames)
    assert st.tolist() == [0, 4, 8, 4, 0, 0]
    assert sizes.tolist()[1:4] == [0, 0, 0]
    for p in (1, 2, 3):
        assert (raw[p * slot:(p + 1) * slot] == CANARY).all(), p
    for p in (0, 4, 5):   # the packet, zeros to the next 4 bytes, then the slot untouched
        end = -(-int(sizes[p]) // 4) * 4
        assert (raw[p * slot + int(sizes[p]):p * slot + end] == 0).all()
        assert (raw[p * slot + end:(p + 1) * slot] == CANARY).all()
    with pytest.raises(pkg.AlacGpuError):   # a slot below the bound
        encode(torch, pkg, planar, cfgs, firsts[:1], frames[:1], slot=pkg.encode_max_packet_bytes(1024, 16, 2) - 16)
    with pytest.raises(pkg.AlacGpuError):   # channels other than the cfg's
        encode(torch, pkg, planar[:1], cfgs, firsts[:1], frames[:1])


@pytest.mark.parametrize("C_,ss", [(2, 16), (1, 24), (2, 24)])
def test_save_load_files(torch, pkg, synth, tmp_path, C_, ss):
    from alac.net_amd import container

    rng = np.random.default_rng(C_ * 100 + ss)
    for T, fl in [(int(rng.integers(1, 4096)), 4096), (4096 * 3, 4096), (int(rng.integers(10000, 30000)), 4096),
                  (int(rng.integers(100, 5000)), 1000)]:
        planar = source(synth, C_, ss, -(-T // 4096), 4096, T - 4096 * (-(-T // 4096) - 1), seed=T)
        pcm = torch.from_numpy(planar).cuda()
        path = tmp_path / f"a_{T}_{fl}.m4a"
        size = pkg.save(str(path), pcm, 48000, sample_size=ss, frame_length=fl)
        data = path.read_bytes()
        assert size == len(data)
        back, rate = pkg.load(data, dtype=torch.int32)
        assert rate == 48000 and torch.equal(back.cpu(), torch.from_numpy(planar))
        f32, _ = pkg.load(data)
        buf = io.BytesIO()
        pkg.save(buf, f32, 48000, sample_size=ss, frame_length=fl)     # load (float32) then save: exact
        assert torch.equal(pkg.load(buf.getvalue(), dtype=torch.int32)[0].cpu(), torch.from_numpy(planar))
        t = container.packet_table(data)
        assert t["num_samples"] == T and int(t["cfg"][0]["max_samples_per_frame"]) == fl
        durations = t["durations"].tolist()
        assert durations == [fl] * (T // fl) + ([T % fl] if T % fl else [])
        at = data.rfind(b"alac")
        cookie = np.frombuffer(data[at + 8:at + 32], dtype=">u4")
        assert int(cookie[3]) == int(t["sizes"].max()) and int(cookie[4]) > 0   # maxFrameBytes, avgBitRate
        with container.AlacContext(io.BytesIO(data), batch_packets=3) as ac:   # the read loop takes the file
            buf, got = bytearray(fl * C_ * (ss // 8) + 64), []
            while True:
                k = ac.Read(buf)
                if k == 0:
                    break
                got.append(bytes(buf[:k]))
        raw = b"".join(got)
        ints = np.frombuffer(raw, np.int16).astype(np.int32) if ss == 16 else \
            (np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32) @ np.array([1, 256, 65536]) ^ 0x800000) - 0x800000
        assert np.array_equal(ints.reshape(-1, C_).T, planar)


def test_save_batch_equals_separate_saves(torch, pkg, synth):
    lengths = [5000, 4096, 17, 12000, 8193]
    Tm = max(lengths)
    planar = np.zeros((len(lengths), 2, Tm), np.int32)
    for f, L in enumerate(lengths):
        planar[f, :, :L] = source(synth, 2, 16, -(-L // 4096), 4096, L - 4096 * (-(-L // 4096) - 1), seed=f + 40)
    planar[0, :, lengths[0]:] = 999          # frames past a file's length are not part of it
    pcm = torch.from_numpy(planar).cuda()
    bufs = [io.BytesIO() for _ in lengths]
    sizes = pkg.save_batch(bufs, pcm, lengths, 44100)
    for f, L in enumerate(lengths):
        one = io.BytesIO()
        pkg.save(one, pcm[f, :, :L].contiguous(), 44100)
        assert bufs[f].getvalue() == one.getvalue() and sizes[f] == len(one.getvalue()), f
    out, lens, _ = pkg.load_batch([b.getvalue() for b in bufs], dtype=torch.int32)
    assert lens.tolist() == lengths
    for f, L in enumerate(lengths):
        assert np.array_equal(out[f, :, :L].cpu().numpy(), planar[f, :, :L])
