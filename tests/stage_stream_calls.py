"""What tests/test_stage_streams.py is made of: the gate that keeps a stream busy for a known time, and one `Call` per stage
entry point -- its true inputs, the buffers the call reads them from, its outputs and the call itself -- so that the same call
can run alone on a fresh context (the reference) and behind a gate on a side stream (the test)."""
import numpy as np

from test_features import header_constant

CFG = [(512, 16, 40, 10, 14, 2)]
SENTINEL = 0x5A          # every byte of an output in front of the call


# ---- the gate ------------------------------------------------------------------------------------------------------------------
_RATE = {}               # how the delay scales: cycles of torch.cuda._sleep, or elementwise ops over _BALLAST, per millisecond
_BALLAST = []


def _delay(torch, amount):
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(amount))
    else:
        for _ in range(int(amount)):
            _BALLAST[0].mul_(1.0)


def calibrate(torch):
    """The delay's unit per millisecond, measured once on the default stream with timing events"""
    if "per_ms" not in _RATE:
        if not hasattr(torch.cuda, "_sleep"):
            _BALLAST.append(torch.ones(1 << 26, dtype=torch.float32, device="cuda"))
        probe = 20_000_000 if hasattr(torch.cuda, "_sleep") else 50
        _delay(torch, probe // 10)                                  # (the first launch of the delay's kernel is not timed)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _delay(torch, probe)
        t1.record()
        t1.synchronize()
        _RATE["per_ms"] = probe / max(t0.elapsed_time(t1), 1e-3)
        print(f"[gate] {'torch.cuda._sleep' if hasattr(torch.cuda, '_sleep') else 'elementwise ops'}: {_RATE['per_ms']:.1f} units per ms")
    return _RATE["per_ms"]


class Gate:
    """A delay of `ms` milliseconds enqueued on `stream`; `event` is recorded behind it.  pending(): the delay has not
    ended.  report(), behind a synchronise, prints and returns the duration the timing events measured."""

    def __init__(self, torch, stream, ms):
        rate = calibrate(torch)
        self.ms = ms
        self.t0, self.event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.t0.record()
            _delay(torch, ms * rate)
            self.event.record()

    def pending(self):
        return not self.event.query()

    def report(self, what=""):
        self.event.synchronize()
        took = self.t0.elapsed_time(self.event)
        print(f"[gate] {what}: asked for {self.ms:.0f} ms, took {took:.1f} ms")
        return took


def too_short(what, gate_ms, enqueue_s):
    return (f"{what}: the gate of {gate_ms:.0f} ms had ended when the enqueues behind it returned ({enqueue_s * 1e3:.2f} ms of host "
            f"time): the delay is too short for this host, nothing was checked")


# ---- a call ----------------------------------------------------------------------------------------------------------------------
class Call:
    """One stage call.  true: name -> the input as it has to be (device tensors); buf: the tensors the call reads, of the
    same shapes; outs: its outputs.  poison() fills buf with NaN (floats) or the wrong constant `wrong[name]` (integers) and
    the outputs with SENTINEL bytes; load() copies the true inputs into buf on the current stream; run(ctx, stream) makes
    the call with `stream` (a raw handle); clones() copies the outputs on the current stream."""

    def __init__(self, torch, true, outs, fn, wrong=None, keep=None):
        self.torch, self.true, self.outs, self.fn, self.wrong, self.keep = torch, true, list(outs), fn, wrong or {}, keep
        self.buf = {k: torch.empty_like(v) for k, v in true.items()}

    def poison(self):
        for k, b in self.buf.items():
            b.fill_(float("nan") if b.dtype.is_floating_point else self.wrong[k])
        for o in self.outs:
            o.view(self.torch.uint8).fill_(SENTINEL)

    def load(self):
        for k, b in self.buf.items():
            b.copy_(self.true[k])

    def run(self, ctx, stream):
        self.fn(ctx, self.buf, self.outs, stream)

    def clones(self):
        return [o.clone() for o in self.outs]


def same_bits(torch, got, want):
    """Two lists of tensors, bit for bit (NaN payloads and the sign of zero included)"""
    return len(got) == len(want) and all(
        g.shape == w.shape and g.dtype == w.dtype and torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8))
        for g, w in zip(got, want))


def alone(torch, pkg, call):
    """The reference of a call: made alone on the default stream of a fresh context behind a full synchronise"""
    call.poison()
    call.load()
    torch.cuda.synchronize()
    with pkg.AlacGpuContext(CFG) as ctx:
        call.run(ctx, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    want = call.clones()
    torch.cuda.synchronize()
    assert not any(bool((w.view(torch.uint8) == SENTINEL).all()) for w in want if w.numel() > 8), "the reference call wrote nothing"
    return want


def _gen(torch, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _randn(torch, shape, seed):
    return torch.randn(shape, generator=_gen(torch, seed), device="cuda", dtype=torch.float32)


def _up(torch, a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to("cuda")      # (every value here fits the signed type)


def _raw(torch, shape, dtype):
    return torch.empty(shape, dtype=dtype, device="cuda")


# ---- the stage calls ---------------------------------------------------------------------------------------------------------------
def plan_call(torch, pkg, each, seed=0, crops=9):
    """The crop planner over test_corpus_plan's hand-made tables: `crops` crops, more than the four of one workgroup"""
    from test_corpus_plan import TABLES, tables_of

    tb = tables_of(TABLES)
    rng = np.random.default_rng(100 + seed)
    totals = [int(np.sum(d)) for d in TABLES]
    cf = rng.integers(0, 6, crops).astype(np.uint32)
    co = np.array([int(rng.integers(0, totals[f] + 1)) for f in cf], dtype=np.uint64)
    L = 4096
    K = max(pkg.entries_per_crop(tb["pkt_end"], tb["file_first"], L), 1)
    d_tab = [_up(torch, tb["pkt_offset"], np.int64), _up(torch, tb["pkt_size"], np.int32), _up(torch, tb["pkt_end"], np.int64),
             _up(torch, tb["file_first"], np.int32), _up(torch, tb["file_cfg"], np.int16)]
    true = dict(crop_file=_up(torch, cf, np.int32), crop_offset=_up(torch, co, np.int64))
    wrong = dict(crop_file=1, crop_offset=3)
    if each:
        true["crop_frames"] = _up(torch, rng.integers(1, L + 1, crops).astype(np.uint32), np.int32)
        wrong["crop_frames"] = 1
    kinds = [torch.int64, torch.int32, torch.int16, torch.int64, torch.int32, torch.int32, torch.int64]
    outs = [_raw(torch, (crops * K,), k) for k in kinds[:6]] + [_raw(torch, (crops,), kinds[6])]

    def fn(ctx, b, o, stream):
        front = [ctx._ctx, *[pkg._dp(t) for t in d_tab], len(tb["file_first"]) - 1, pkg._dp(b["crop_file"]), pkg._dp(b["crop_offset"])]
        back = [crops, L, K, 2 * L, *[pkg._dp(t) for t in o], pkg._VP(stream)]
        if each:
            rc = pkg.lib().alacgpu_plan_crops_frames_device(*front, pkg._dp(b["crop_frames"]), *back)
        else:
            rc = pkg.lib().alacgpu_plan_crops_device(*front, *back)
        assert rc == 0, rc

    return Call(torch, true, outs, fn, wrong, keep=d_tab)


def scan_tile():
    return header_constant("ALAC_SCAN_THREADS", "alac_corpus.h") * header_constant("ALAC_SCAN_ITEMS", "alac_corpus.h")


def scan_need(n):
    """The scratch bytes of a scan over n sizes (scan_sizes of alacgpu_stages.hip)"""
    tile = scan_tile()
    t1 = -(-n // tile)
    t2 = -(-t1 // tile)
    return 8 * (t1 + t2) if t1 > 1 else 0


def compact_call(torch, pkg, n, seed=0):
    """The packet compaction over n 16-byte slots of 0 .. 6 bytes each; the blob holds at most 1 MiB of them"""
    slot, base = 16, 9
    g = _gen(torch, 200 + seed)
    true = dict(sizes=torch.randint(0, 7, (n,), generator=g, device="cuda", dtype=torch.int32),
                packets=torch.randint(0, 256, (n * slot,), generator=g, device="cuda", dtype=torch.uint8))
    capacity = min(base + 7 * n + 40, 1 << 20)
    outs = [_raw(torch, (capacity,), torch.uint8), _raw(torch, (n,), torch.int64), _raw(torch, (1,), torch.int64)]

    def fn(ctx, b, o, stream):
        ctx.compact_packets_device(b["packets"], slot, b["sizes"], n, o[0], base, capacity, o[1], o[2], stream=stream)

    return Call(torch, true, outs, fn, dict(sizes=1, packets=0x33))


def stage_call(torch, pkg, n, seed=0):
    """The packet staging of n packets of 0 .. 19 bytes out of a device blob of 70000 bytes; the staging blob holds at most
    1 MiB of them"""
    lo_bytes = 70000
    g = _gen(torch, 300 + seed)
    true = dict(blob=torch.randint(0, 256, (lo_bytes + 32,), generator=g, device="cuda", dtype=torch.uint8),
                src_offset=torch.randint(0, lo_bytes - 32, (n,), generator=g, device="cuda", dtype=torch.int64),
                sizes=torch.randint(0, 20, (n,), generator=g, device="cuda", dtype=torch.int32))
    capacity = min(32 * n + 64, 1 << 20)
    outs = [_raw(torch, (capacity,), torch.uint8), _raw(torch, (n,), torch.int64), _raw(torch, (1,), torch.int64)]

    def fn(ctx, b, o, stream):
        ctx.stage_packets_device(b["blob"], lo_bytes, None, 0, b["src_offset"], b["sizes"], n, o[0], capacity, o[1], o[2], stream=stream)

    return Call(torch, true, outs, fn, dict(blob=0x33, src_offset=16, sizes=1))


def _resample_rows(torch, rows, stride, seed):
    true = dict(src=_randn(torch, (rows, 2, stride), 400 + seed), valid=torch.full((rows,), stride, dtype=torch.int64, device="cuda"))
    zeros = torch.zeros(rows, dtype=torch.int64, device="cuda")
    return true, zeros, dict(valid=0)


def resample_frames():
    return header_constant("ALAC_RESAMPLE_MAX_TILE", "alac_resample.h") + 1         # one tile plus one frame


def resample_call(torch, pkg, seed=0, rows=2):
    from alac.net_amd.resample import resample_table

    a, b, width, d0, w = resample_table(44100, 16000)
    frames = resample_frames()
    stride = frames * a // b + 2 * width + 8
    true, zeros, wrong = _resample_rows(torch, rows, stride, seed)
    d_d0, d_w = _up(torch, d0, np.int32), _up(torch, w, np.float32)
    outs = [_raw(torch, (rows, 2, frames), torch.float32)]

    def fn(ctx, bf, o, stream):
        ctx.resample_device(bf["src"], rows, 2, stride, zeros, bf["valid"], zeros, frames, a, b, width, d_d0, d_w, False, o[0], stream=stream)

    return Call(torch, true, outs, fn, wrong, keep=(d_d0, d_w, zeros))


def resample_rows_call(torch, pkg, seed=0):
    from test_resample_rows import Tables

    tabs = Tables(torch, [44100, 48000, 16000], 16000)            # 441 : 160, 3 : 1 and the table that copies
    rows, frames = 3, resample_frames()
    stride = frames * 3 + 200
    true, zeros, wrong = _resample_rows(torch, rows, stride, seed)
    true["row_table"] = _up(torch, np.array([0, 1, 2], np.int32), np.int32)
    wrong["row_table"] = 2
    outs = [_raw(torch, (rows, 2, frames), torch.float32)]

    def fn(ctx, bf, o, stream):
        ctx.resample_rows_device(bf["src"], rows, 2, stride, zeros, bf["valid"], zeros, frames, tabs.desc, tabs.d_desc, tabs.d_d0, tabs.d_w,
                                 bf["row_table"], False, o[0], stream=stream)

    return Call(torch, true, outs, fn, wrong, keep=(tabs, zeros))


def resample_ratio_rows_call(torch, pkg, seed=0):
    from alac.net_amd.resample import filter_width

    ratios = np.array([(9, 10, filter_width(9, 10)), (11, 10, filter_width(11, 10))], dtype=np.uint32)
    rows, frames = 2, resample_frames()
    stride = frames * 11 // 10 + 200
    true, zeros, wrong = _resample_rows(torch, rows, stride, seed)
    true["row_ratio"] = _up(torch, np.array([0, 1], np.int32), np.int32)
    wrong["row_ratio"] = 0
    d_ratios = _up(torch, ratios.view(np.int32), np.int32)
    outs = [_raw(torch, (rows, 2, frames), torch.float32)]

    def fn(ctx, bf, o, stream):
        ctx.resample_ratio_rows_device(bf["src"], rows, 2, stride, zeros, bf["valid"], zeros, frames, ratios, d_ratios, bf["row_ratio"], False,
                                       o[0], stream=stream)

    return Call(torch, true, outs, fn, wrong, keep=(d_ratios, zeros))


def transform_call(torch, pkg, spec, lines, seed=0, rows=2, T=2000):
    """log-mel, Kaldi fbank or MFCC of [rows, 1, T] through the specification's own launch; lines: n_mels or n_ceps"""
    true = dict(src=0.1 * _randn(torch, (rows, 1, T), 500 + seed))
    spec.device_tables(torch.device("cuda", 0))
    outs = [_raw(torch, (rows, 1, lines, int(spec.frames(T))), torch.float32)]

    def fn(ctx, b, o, stream):
        spec.launch(ctx, b["src"], rows, 1, T, T, o[0], stream)

    return Call(torch, true, outs, fn)


def deltas_call(torch, pkg, seed=0):
    spec = pkg.Deltas(2, 2)
    B, C, F, T = 2, 1, 5, 300
    true = dict(feats=_randn(torch, (B, C, F, T), 600 + seed))
    scales = spec.device_scales(torch.device("cuda", 0))
    outs = [_raw(torch, (B, C, spec.lines(F), T), torch.float32)]

    def fn(ctx, b, o, stream):
        ctx.deltas_device(b["feats"], o[0], B, C, F, T, T, T, None, spec.order, spec.window, scales, stream=stream)

    return Call(torch, true, outs, fn)


def meanvar_call(torch, pkg, line_len, seed=0):
    rows, lines = 2, 3
    true = dict(x=_randn(torch, (rows, lines, line_len), 700 + seed) + 2.0, valid=_up(torch, [line_len, line_len - 7], np.int64))
    outs = [_raw(torch, (rows, lines, line_len), torch.float32)]

    def fn(ctx, b, o, stream):
        ctx.normalize_meanvar_device(b["x"], o[0], rows, lines, line_len, line_len, b["valid"], True, True, 1e-5, stream=stream)

    return Call(torch, true, outs, fn, dict(valid=1))


def top_need(rows, row_elems):
    part, most = header_constant("ALAC_TOP_PART", "alac_normalize.h"), header_constant("ALAC_TOP_MAX_PARTS", "alac_normalize.h")
    assert row_elems <= part * most
    return 4 * rows * -(-row_elems // part)


def top_call(torch, pkg, row_elems, seed=0, rows=2):
    true = dict(x=_randn(torch, (rows, 1, row_elems), 800 + seed))
    outs = [_raw(torch, (rows, 1, row_elems), torch.float32)]

    def fn(ctx, b, o, stream):
        ctx.normalize_top_device(b["x"], o[0], rows, 1, row_elems, row_elems, 1.5, 0.25, 1.0, False, stream=stream)

    return Call(torch, true, outs, fn)


def specaugment_call(torch, pkg, seed=0):
    B, C, M, N = 2, 1, 8, 300
    true = dict(x=_randn(torch, (B, C, M, N), 900 + seed), warp=_up(torch, [[150, 153], [100, 96]], np.int32),
                freq=_up(torch, [[[1, 2]], [[5, 3]]], np.int32), time=_up(torch, [[[10, 20]], [[200, 50]]], np.int32))
    outs = [_raw(torch, (B, C, M, N), torch.float32)]

    def fn(ctx, b, o, stream):
        ctx.specaugment_device(b["x"], o[0], B, C, M, N, N, None, b["warp"], b["freq"], b["time"], -1.0, stream=stream)

    return Call(torch, true, outs, fn, dict(warp=0, freq=0, time=0))


def mix_need(rows, frames):
    part, most = header_constant("ALAC_MIX_PART", "alac_mix.h"), header_constant("ALAC_MIX_MAX_PARTS", "alac_mix.h")
    assert frames <= part * most
    return 8 * rows * -(-frames // part)


def mix_call(torch, pkg, frames, seed=0, rows=2):
    true = dict(x=_randn(torch, (rows, 2, frames), 1000 + seed), noise=_randn(torch, (rows, 1, frames), 1100 + seed),
                ratio=torch.rand(rows, generator=_gen(torch, 1200 + seed), device="cuda", dtype=torch.float32) + 0.1)
    outs = [_raw(torch, (rows, 2, frames), torch.float32)]

    def fn(ctx, b, o, stream):
        ctx.mix_device(b["x"], o[0], b["noise"], rows, 2, 1, frames, frames, frames, None, None, b["ratio"], stream=stream)

    return Call(torch, true, outs, fn)


def reverb_frames():
    return header_constant("ALAC_REVERB_N", "alac_reverb.h") // 2 + 1               # H + 1: two blocks, two partitions


def reverb_spectra(rows):
    """The bytes of the spectra in a reverb call's scratch (one channel, reverb_frames() frames of signal and response); the
    rows' verdicts behind them are at most 64 bytes a row"""
    N = header_constant("ALAC_REVERB_N", "alac_reverb.h")
    H = N // 2
    f = reverb_frames()
    units = (-(-f // H) + 1) + -(-f // H)
    return 8 * N * units * rows


def reverb_call(torch, pkg, seed=0, rows=2):
    f = reverb_frames()
    decay = torch.exp(-torch.arange(f, device="cuda", dtype=torch.float32) / 300.0)
    true = dict(x=_randn(torch, (rows, 1, f), 1300 + seed), rir=_randn(torch, (rows, 1, f), 1400 + seed) * decay)
    outs = [_raw(torch, (rows, 1, f), torch.float32)]

    def fn(ctx, b, o, stream):
        ctx.reverb_device(b["x"], o[0], b["rir"], rows, 1, 1, f, f, f, f, None, None, stream=stream)

    return Call(torch, true, outs, fn)


def encode_call(torch, pkg, n, seed=0):
    """n packets of up to 512 frames by test_encode_policy.run's recipe: its output tensors and canary, its argument order"""
    import test_encode as te
    import test_encode_policy as tep

    cfg = CFG[0]
    T = 512 * n
    x = np.arange(T)
    rng = np.random.default_rng(1500 + seed)
    planar = np.stack([np.round(8000 * np.sin(0.003 * x) + rng.normal(0, 200, T)),
                       np.round(6000 * np.sin(0.005 * x) + rng.normal(0, 200, T))]).astype(np.int32)
    firsts, frames = te.split(T, 512)
    firsts, frames = firsts + 3, frames - 3
    slot = pkg.encode_max_packet_bytes(cfg[0], cfg[1], 2)
    true = dict(pcm=torch.from_numpy(planar).cuda())
    fixed = (_up(torch, np.asarray(firsts, np.int64), np.int64), _up(torch, np.asarray(frames, np.int32), np.int32),
             torch.zeros(n, dtype=torch.int16, device="cuda"))
    outs = [_raw(torch, (n * slot,), torch.uint8), _raw(torch, (n,), torch.int32), _raw(torch, (n,), torch.int32)]

    def fn(ctx, b, o, stream):
        ctx.encode_device(b["pcm"], 2, *fixed, n, o[0], slot, o[1], o[2], layout="planar", plane_stride=T, stream=stream)

    call = Call(torch, true, outs, fn, dict(pcm=12345), keep=fixed)
    call.policy = lambda: tep.run(torch, pkg, true["pcm"], 2, [cfg], firsts, frames, plane_stride=T)     # the same call through `run`
    call.unpack = lambda got: tep.unpack(got[0], got[1], got[2], slot)
    return call

