"""The argument contract of every device entry point of include/alacgpu.h, as one table: the smallest call each accepts, and
one perturbation at a time of it -- a NULL, a pointer at half its alignment, a scalar out of range, no work -- with the return
code the header promises; where the header is silent (the order of the checks against the returns for no work) the code the
library gave when this file was written, which is what a caller has seen since.  A refused call must return -1, enqueue
nothing -- every output keeps its sentinel bytes -- and leave alacgpu_last_error as it was.  What the accepted calls compute
is the other test files' business."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = [(16, 16, 40, 10, 14, 1)]         # one mono 16-bit stream of 16-frame packets: Smax 16
NULL, MIS = "NULL", "half its alignment"
INF, NAN = float("inf"), float("nan")
SENTINEL = 0x5A

# the alignment a pointer argument needs (include/alacgpu.h); every other pointer needs 4
ALIGN = {**{k: 16 for k in ("d_blob", "d_packets", "d_stage", "d_blob_lo", "blob_hi")},
         **{k: 8 for k in ("d_offsets", "d_dst_first", "d_pkt_offset", "d_pkt_end", "d_crop_offset", "d_lengths", "d_total",
                           "d_src_offset", "d_stage_offset", "d_src_origin", "d_src_valid", "d_out_first", "d_src_first")},
         **{k: 2 for k in ("d_cfg_idx", "d_file_cfg")}}

ARGS = {
    "decode_batch": "ctx d_blob blob_bytes d_offsets d_sizes d_cfg_idx n_packets d_pcm_out slot_ints d_out_bytes d_out_samples "
                    "d_status stream",
    "decode_into": "ctx d_blob blob_bytes d_offsets d_sizes d_cfg_idx n_packets d_dst_first d_dst_frames d_out out_elems channels "
                   "layout dtype plane_stride d_out_samples d_status stream",
    "decode_window_into": "ctx d_blob blob_bytes d_offsets d_sizes d_cfg_idx n_packets d_dst_first d_dst_frames d_src_skip d_out "
                          "out_elems channels layout dtype plane_stride d_out_samples d_status stream",
    "plan_crops": "ctx d_pkt_offset d_pkt_size d_pkt_end d_file_first d_file_cfg n_files d_crop_file d_crop_offset n_crops "
                  "crop_frames entries_per_crop dst_stride d_offsets d_sizes d_cfg_idx d_dst_first d_dst_frames d_src_skip "
                  "d_lengths stream",
    "plan_crops_frames": "ctx d_pkt_offset d_pkt_size d_pkt_end d_file_first d_file_cfg n_files d_crop_file d_crop_offset "
                         "d_crop_frames n_crops crop_frames entries_per_crop dst_stride d_offsets d_sizes d_cfg_idx d_dst_first "
                         "d_dst_frames d_src_skip d_lengths stream",
    "compact_packets": "ctx d_packets slot_bytes d_sizes n_packets d_blob base blob_capacity d_pkt_offset d_total stream",
    "stage_packets": "ctx d_blob_lo lo_bytes blob_hi hi_bytes d_src_offset d_sizes n_packets d_stage stage_capacity d_stage_offset "
                     "d_total stream",
    "resample": "ctx d_src rows channels src_stride d_src_origin d_src_valid d_out_first out_frames a b width d_d0 d_weights mono "
                "d_out stream",
    "resample_rows": "ctx d_src rows channels src_stride d_src_origin d_src_valid d_out_first out_frames tables d_tables n_tables "
                     "d_d0 d_weights d_row_table mono d_out stream",
    "logmel": "ctx d_src rows channels src_stride frames n_fft hop n_mels d_window d_basis d_fb log_mode floor d_out out_frames "
              "stream",
    "encode": "ctx d_pcm src_elems channels layout dtype plane_stride d_src_first d_src_frames d_cfg_idx n_packets d_packets "
              "slot_bytes d_sizes d_status stream",
}

# (entry point, arguments, perturbation, expected return code).  Arguments as one string: each of them alone gets the
# perturbation; as a tuple: all of them together, each its own.  A perturbation is NULL, MIS (the pointer moved up by half the
# alignment it needs), DEVICE / HOST (for blob_hi: 16 bytes of device memory, of ordinary host memory) or the argument's value.
DEVICE, HOST = "device memory", "ordinary host memory"
DECODE_INTO = [   # both alacgpu_decode_into_device and alacgpu_decode_window_into_device
    ("ctx d_blob d_offsets d_sizes d_dst_first d_dst_frames d_out d_status", NULL, -1),
    ("d_cfg_idx d_out_samples", NULL, 0),
    ("d_blob d_offsets d_sizes d_cfg_idx d_dst_first d_dst_frames d_out d_out_samples d_status", MIS, -1),
    ("channels", 0, -1), ("channels", 3, -1),
    ("layout", 2, -1), ("layout", -1, -1), ("dtype", 2, -1), ("dtype", -1, -1),
    ("layout", 1, -1),                            # planar with plane_stride 0
    (("layout", "plane_stride"), (1, 16), 0),
    ("n_packets", 0, 0),
    # no work: the view and every array are checked all the same
    (("n_packets", "d_blob"), (0, NULL), -1), (("n_packets", "d_dst_first"), (0, NULL), -1), (("n_packets", "d_status"), (0, NULL), -1),
    (("n_packets", "d_out"), (0, NULL), -1), (("n_packets", "d_offsets"), (0, MIS), -1), (("n_packets", "channels"), (0, 0), -1),
    (("n_packets", "layout"), (0, 1), -1), (("n_packets", "d_cfg_idx"), (0, NULL), 0),
]
PLAN = [          # both planner entry points
    ("ctx d_pkt_offset d_pkt_size d_pkt_end d_file_first d_file_cfg d_crop_file d_crop_offset d_offsets d_sizes d_cfg_idx "
     "d_dst_first d_dst_frames d_src_skip d_lengths", NULL, -1),
    ("d_pkt_offset d_pkt_size d_pkt_end d_file_first d_file_cfg d_crop_file d_crop_offset d_offsets d_sizes d_cfg_idx "
     "d_dst_first d_dst_frames d_src_skip d_lengths", MIS, -1),
    ("entries_per_crop", 0, -1),
    (("n_crops", "entries_per_crop"), (65536, 65536), -1),       # 2^32 entries
    ("n_crops", 0, 0),
    # no crops: nothing but the ctx is looked at
    (("n_crops", "ctx"), (0, NULL), -1), (("n_crops", "entries_per_crop"), (0, 0), 0), (("n_crops", "d_pkt_offset"), (0, NULL), 0),
    (("n_crops", "d_lengths"), (0, NULL), 0), (("n_crops", "d_offsets"), (0, MIS), 0),
]
RESAMPLE = [      # what the two resamplers share
    ("ctx d_src d_src_origin d_src_valid d_out_first d_d0 d_weights d_out", NULL, -1),
    ("d_src d_src_origin d_src_valid d_out_first d_d0 d_weights d_out", MIS, -1),
    ("channels", 0, -1), ("channels", 3, -1), ("mono", 1, 0),
    ("out_frames", 1 << 62, -1),                  # 2^31 tiles and more
    ("rows", 0, 0), ("out_frames", 0, 0),
    # no work: every argument is checked all the same
    (("rows", "d_src"), (0, NULL), -1), (("rows", "d_out"), (0, MIS), -1), (("out_frames", "channels"), (0, 3), -1),
    (("out_frames", "d_weights"), (0, NULL), -1),
]
CASES = [
    *[("decode_batch", *c) for c in [
        ((), (), 0),
        ("ctx d_blob d_offsets d_sizes d_pcm_out d_status", NULL, -1),
        ("d_cfg_idx d_out_bytes d_out_samples", NULL, 0),
        ("d_blob d_offsets d_sizes d_cfg_idx d_pcm_out d_out_bytes d_out_samples d_status", MIS, -1),
        ("slot_ints", 0, -1),
        ("n_packets", 0, 0),
        # no packets: nothing but the ctx is looked at
        (("n_packets", "ctx"), (0, NULL), -1), (("n_packets", "slot_ints"), (0, 0), 0), (("n_packets", "d_blob"), (0, MIS), 0),
        (("n_packets", "d_blob", "d_offsets", "d_sizes", "d_pcm_out", "d_status"), (0, NULL, NULL, NULL, NULL, NULL), 0),
    ]],
    *[("decode_into", *c) for c in [((), (), 0), *DECODE_INTO]],
    *[("decode_window_into", *c) for c in [
        ((), (), 0), *DECODE_INTO,
        ("d_src_skip", NULL, 0), ("d_src_skip", MIS, -1), (("n_packets", "d_src_skip"), (0, MIS), -1),
    ]],
    *[("plan_crops", *c) for c in [((), (), 0), *PLAN]],
    *[("plan_crops_frames", *c) for c in [
        ((), (), 0), *PLAN,
        ("d_crop_frames", NULL, -1), ("d_crop_frames", MIS, -1), (("n_crops", "d_crop_frames"), (0, NULL), 0),
    ]],
    *[("compact_packets", *c) for c in [
        ((), (), 0),
        ("ctx d_packets d_sizes d_blob d_pkt_offset d_total", NULL, -1),
        ("d_packets d_sizes d_pkt_offset d_total", MIS, -1),
        ("d_blob", MIS, 0),                           # the blob is byte granular
        ("slot_bytes", 0, -1), ("slot_bytes", 8, -1), ("slot_bytes", 24, -1),
        ("n_packets", 0, 0),
        # no packets: d_total and slot_bytes are checked, d_total[0] becomes 0, nothing else is looked at
        (("n_packets", "ctx"), (0, NULL), -1), (("n_packets", "d_total"), (0, NULL), -1), (("n_packets", "d_total"), (0, MIS), -1),
        (("n_packets", "slot_bytes"), (0, 0), -1), (("n_packets", "slot_bytes"), (0, 8), -1), (("n_packets", "d_packets"), (0, MIS), 0),
        (("n_packets", "d_packets", "d_sizes", "d_blob", "d_pkt_offset"), (0, NULL, NULL, NULL, NULL), 0),
    ]],
    *[("stage_packets", *c) for c in [
        ((), (), 0),
        ("ctx d_blob_lo d_src_offset d_sizes d_stage d_stage_offset d_total", NULL, -1),
        (("d_blob_lo", "lo_bytes"), (NULL, 0), 0),    # either part may be NULL with 0 bytes (blob_hi is, in the smallest call)
        (("blob_hi", "hi_bytes"), (NULL, 16), -1), (("blob_hi", "hi_bytes"), (DEVICE, 16), 0),
        (("blob_hi", "hi_bytes"), (HOST, 16), -1),    # neither device memory nor page-locked
        ("d_blob_lo blob_hi d_src_offset d_sizes d_stage d_stage_offset d_total", MIS, -1),
        (("blob_hi", "hi_bytes"), (MIS, 16), -1),
        (("blob_hi", "hi_bytes", "lo_bytes"), (DEVICE, 16, (1 << 64) - 1), -1),     # the address space does not fit 64 bits
        ("n_packets", 0, 0),
        # no packets: d_total and the two bases are checked, d_total[0] becomes 0, nothing else is looked at
        (("n_packets", "ctx"), (0, NULL), -1), (("n_packets", "d_total"), (0, NULL), -1), (("n_packets", "d_total"), (0, MIS), -1),
        (("n_packets", "d_blob_lo"), (0, NULL), -1), (("n_packets", "d_blob_lo"), (0, MIS), -1),
        (("n_packets", "blob_hi", "hi_bytes"), (0, NULL, 16), -1), (("n_packets", "d_stage"), (0, MIS), 0),
        (("n_packets", "blob_hi", "hi_bytes", "lo_bytes"), (0, DEVICE, 16, (1 << 64) - 1), 0),
        (("n_packets", "d_src_offset", "d_sizes", "d_stage", "d_stage_offset"), (0, NULL, NULL, NULL, NULL), 0),
    ]],
    *[("resample", *c) for c in [
        ((), (), 0), *RESAMPLE,
        ("a", 0, -1), ("b", 0, -1), ("width", 0, -1),
        ("b", 5462, -1),                              # 3 * 5462 weights: above ALAC_RESAMPLE_MAX_TABLE (16384)
        (("b", "width"), (1, 8192), -1),
        (("rows", "a"), (0, 0), -1), (("out_frames", "b"), (0, 5462), -1),
    ]],
    *[("resample_rows", *c) for c in [
        ((), (), 0), *RESAMPLE,
        ("tables d_tables d_row_table", NULL, -1), ("tables d_tables d_row_table", MIS, -1),
        ("n_tables", 0, -1),
        ("tables", [0, 2, 1, 0, 0], -1), ("tables", [1, 0, 1, 0, 0], -1), ("tables", [1, 2, 0, 0, 0], -1),
        ("tables", [1, 5462, 1, 0, 0], -1), ("tables", [1, 1, 8192, 0, 0], -1),
        (("rows", "n_tables"), (0, 0), -1), (("rows", "tables"), (0, [0, 2, 1, 0, 0]), -1), (("out_frames", "tables"), (0, NULL), -1),
    ]],
    *[("logmel", *c) for c in [
        ((), (), 0),
        ("ctx d_src d_window d_basis d_fb d_out", NULL, -1),
        ("d_src d_window d_basis d_fb d_out", MIS, -1),
        ("n_fft", 15, -1), ("n_fft", 2049, -1), ("hop", 0, -1), ("hop", 17, -1), ("n_mels", 0, -1), ("n_mels", 257, -1),
        ("channels", 0, -1),
        ("floor", 0.0, -1), ("floor", -1.0, -1), ("floor", INF, -1), ("floor", NAN, -1),
        ("log_mode", 3, -1), ("log_mode", -1, -1), ("log_mode", 0, 0), ("log_mode", 2, 0),
        ("out_frames", 4, -1), ("out_frames", 6, -1),
        ("frames", 8, -1),                            # frames <= n_fft / 2
        ("frames", 17, -1),                           # frames above src_stride (1 + 17 / 4 is still 5)
        ("rows", 0, 0),
        # no rows: every argument is checked all the same
        (("rows", "d_src"), (0, NULL), -1), (("rows", "d_out"), (0, MIS), -1), (("rows", "n_fft"), (0, 15), -1),
        (("rows", "floor"), (0, NAN), -1), (("rows", "out_frames"), (0, 4), -1),
    ]],
    *[("encode", *c) for c in [
        ((), (), 0),
        ("ctx d_pcm d_src_first d_src_frames d_cfg_idx d_packets d_sizes d_status", NULL, -1),
        ("d_pcm d_src_first d_src_frames d_cfg_idx d_packets d_sizes d_status", MIS, -1),
        ("channels", 0, -1), ("channels", 3, -1),
        ("channels", 2, -1),                          # not the channels of the ctx's cfg
        ("layout", 2, -1), ("dtype", 2, -1), ("layout", 1, -1), (("layout", "plane_stride"), (1, 16), 0),
        ("slot_bytes", 0, -1), ("slot_bytes", 8, -1), ("slot_bytes", 56, -1),
        ("slot_bytes", 32, -1),                       # alacgpu_encode_max_packet_bytes(16, 16, 1) is 48
        ("slot_bytes", 64, 0),
        ("n_packets", 0, 0),
        # no packets: every argument is checked all the same
        (("n_packets", "d_pcm"), (0, NULL), -1), (("n_packets", "d_status"), (0, NULL), -1), (("n_packets", "d_packets"), (0, MIS), -1),
        (("n_packets", "channels"), (0, 2), -1), (("n_packets", "slot_bytes"), (0, 32), -1), (("n_packets", "layout"), (0, 1), -1),
    ]],
]


class Arena:
    """Buffers carved out of one uint8 device tensor, 256 bytes apart at least; addresses as integers."""

    def __init__(self, torch, nbytes):
        self.torch, self.bytes, self.used = torch, torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), 0
        assert self.bytes.data_ptr() % 256 == 0

    def room(self, nbytes):
        at, self.used = self.used, self.used + (nbytes + 16 + 255) // 256 * 256      # (+ 16: a pointer may move up by 8)
        assert self.used <= self.bytes.numel()
        return at

    def put(self, values, dtype):
        a = np.ascontiguousarray(np.asarray(values, dtype=dtype)).reshape(-1).view(np.uint8)
        at = self.room(a.size)
        self.bytes[at:at + a.size] = self.torch.from_numpy(a.copy()).to("cuda")
        return self.bytes.data_ptr() + at


def smallest_calls(torch, pkg, synth, ctx, src, out):
    """Per entry point the arguments of the smallest call it accepts (pointers as integer addresses), inputs in `src` and
    every output in `out`; and where d_total lies in `out` for the two entry points that have one."""
    inp = lambda values, dtype: src.put(values, dtype)
    res = lambda nbytes: out.bytes.data_ptr() + out.room(nbytes)
    packet = np.frombuffer(synth.encode_packet(synth.packet_descs(1, n=16, max_samples_per_frame=16, stereo=0),
                                               (np.arange(16) * 37 - 300).astype(np.int32)), dtype=np.uint8)
    blob = np.zeros((packet.size + 15) // 16 * 16 + 64, dtype=np.uint8)
    blob[:packet.size] = packet
    decode = dict(ctx=ctx, d_blob=inp(blob, np.uint8), blob_bytes=packet.size, d_offsets=inp([0], np.uint64), d_sizes=inp([packet.size], np.uint32),
                  d_cfg_idx=inp([0], np.uint16), n_packets=1, stream=None)
    into = dict(decode, d_dst_first=inp([0], np.uint64), d_dst_frames=inp([16], np.uint32), d_out=res(64), out_elems=16, channels=1,
                layout=0, dtype=0, plane_stride=0, d_out_samples=res(4), d_status=res(4))
    plan = dict(ctx=ctx, d_pkt_offset=inp([0], np.uint64), d_pkt_size=inp([16], np.uint32), d_pkt_end=inp([16], np.uint64),
                d_file_first=inp([0, 1], np.uint32), d_file_cfg=inp([0], np.uint16), n_files=1, d_crop_file=inp([0], np.uint32),
                d_crop_offset=inp([0], np.uint64), n_crops=1, crop_frames=16, entries_per_crop=1, dst_stride=16, d_offsets=res(8),
                d_sizes=res(4), d_cfg_idx=res(2), d_dst_first=res(8), d_dst_frames=res(4), d_src_skip=res(4), d_lengths=res(8), stream=None)
    table = [1, 2, 1, 0, 0]                                     # 1 : 2 at width 1: d0 = floor(i / 2) - 1, three weights per phase
    resample = dict(ctx=ctx, d_src=inp(np.ones(4), np.float32), rows=1, channels=1, src_stride=4, d_src_origin=inp([0], np.int64),
                    d_src_valid=inp([4], np.int64), d_out_first=inp([0], np.int64), out_frames=4, a=1, b=2, width=1,
                    d_d0=inp([-1, -1], np.int32), d_weights=inp([0, 1, 0, 0, .5, .5], np.float32), mono=0, d_out=res(16), stream=None)
    rows = {k: v for k, v in resample.items() if k not in ("a", "b", "width")}
    rows.update(tables=table, d_tables=inp(table, np.uint32), n_tables=1, d_row_table=inp([0], np.uint32))
    total = {"compact_packets": out.room(8), "stage_packets": out.room(8)}
    at = lambda name: out.bytes.data_ptr() + total[name]
    calls = {
        "decode_batch": dict(decode, d_pcm_out=res(64), slot_ints=16, d_out_bytes=res(4), d_out_samples=res(4), d_status=res(4)),
        "decode_into": into,
        "decode_window_into": dict(into, d_src_skip=inp([0], np.uint32)),
        "plan_crops": plan,
        "plan_crops_frames": dict(plan, d_crop_frames=inp([16], np.uint32)),
        "compact_packets": dict(ctx=ctx, d_packets=inp(np.arange(16), np.uint8), slot_bytes=16, d_sizes=inp([16], np.uint32), n_packets=1,
                                d_blob=res(64), base=0, blob_capacity=16, d_pkt_offset=res(8), d_total=at("compact_packets"), stream=None),
        "stage_packets": dict(ctx=ctx, d_blob_lo=inp(np.arange(16), np.uint8), lo_bytes=16, blob_hi=None, hi_bytes=0,
                              d_src_offset=inp([0], np.uint64), d_sizes=inp([16], np.uint32), n_packets=1, d_stage=res(64),
                              stage_capacity=16, d_stage_offset=res(8), d_total=at("stage_packets"), stream=None),
        "resample": resample,
        "resample_rows": rows,
        "logmel": dict(ctx=ctx, d_src=inp(np.ones(16), np.float32), rows=1, channels=1, src_stride=16, frames=16, n_fft=16, hop=4,
                       n_mels=1, d_window=inp(np.ones(16), np.float32), d_basis=inp(np.ones(16 * 18), np.float32),
                       d_fb=inp(np.ones(9), np.float32), log_mode=1, floor=1e-10, d_out=res(4 * 5), out_frames=5, stream=None),
        "encode": dict(ctx=ctx, d_pcm=inp(np.arange(16), np.int32), src_elems=16, channels=1, layout=0, dtype=0, plane_stride=0,
                       d_src_first=inp([0], np.uint64), d_src_frames=inp([16], np.uint32), d_cfg_idx=inp([0], np.uint16), n_packets=1,
                       d_packets=res(64), slot_bytes=48, d_sizes=res(4), d_status=res(4), stream=None),
    }
    return calls, total


def test_every_device_entry_point_checks_what_the_header_promises(synth):
    import torch

    import alac.net_amd as pkg

    L = pkg.lib()
    assert L.alacgpu_encode_max_packet_bytes(16, 16, 1) == 48
    keep = []                                                   # host arrays a call points to

    def host_pointer(values, dtype, offset=0):
        raw = np.zeros(256, dtype=np.uint8)
        keep.append(raw)
        at = -raw.ctypes.data % 16 + offset
        a = np.asarray(values, dtype=dtype).reshape(-1).view(np.uint8)
        raw[at:at + a.size] = a
        return raw.ctypes.data + at

    with pkg.AlacGpuContext(CFG) as gpu:
        src, out = Arena(torch, 1 << 15), Arena(torch, 1 << 15)
        spare = src.put(np.arange(32), np.uint8)                # (what DEVICE stands for)
        calls, total = smallest_calls(torch, pkg, synth, gpu._ctx.value, src, out)
        assert sorted(calls) == sorted(ARGS) and {c[0] for c in CASES} == set(ARGS)
        wrong = []
        for entry, names, changes, want in CASES:
            singly = isinstance(names, str)
            for case in ([((n,), (changes,)) for n in names.split()] if singly else [(names, changes)]):
                args = dict(calls[entry])
                assert set(case[0]) <= set(args), (entry, case)
                for name, change in zip(*case):
                    need = ALIGN.get(name, 4)
                    if name == "tables" and isinstance(change, list):
                        change = host_pointer(change, np.uint32)
                    elif name == "tables" and change is MIS:
                        change = host_pointer(args[name], np.uint32, 2)
                    elif change is MIS:
                        change = (spare if args[name] is None else args[name]) + need // 2
                    elif change is DEVICE:
                        change = spare
                    elif change is HOST:
                        change = host_pointer(np.arange(16), np.uint8)
                    args[name] = None if change is NULL else change
                if isinstance(args.get("tables"), list):
                    args["tables"] = host_pointer(args["tables"], np.uint32)
                out.bytes.fill_(SENTINEL)
                torch.cuda.synchronize()
                before = L.alacgpu_last_error(gpu._ctx)
                rc = getattr(L, f"alacgpu_{entry}_device")(*[args[k] for k in ARGS[entry].split()])
                torch.cuda.synchronize()
                what = (entry, *case, "returned", rc, "expected", want)
                if rc != want:
                    wrong.append(what)
                elif rc != 0:                                   # refused: nothing ran, nothing was noted
                    if not bool((out.bytes == SENTINEL).all()):
                        wrong.append((*what, "and wrote to an output"))
                    if L.alacgpu_last_error(gpu._ctx) != before:
                        wrong.append((*what, "and changed alacgpu_last_error"))
                elif entry in total and args["n_packets"] == 0:  # no packets: d_total[0] = 0 and nothing else
                    got = out.bytes.cpu().numpy()
                    t = total[entry]
                    if got[t:t + 8].any() or not (np.delete(got, np.s_[t:t + 8]) == SENTINEL).all():
                        wrong.append((*what, "and d_total[0] is not 0, or something else was written"))
        assert not wrong, "\n".join(map(str, wrong))
