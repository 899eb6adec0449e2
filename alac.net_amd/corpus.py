"""A corpus of M4A files kept compressed in HBM, and random crops of it decoded without host work per step.

`Corpus` demuxes every file once, uploads the packet bytes and the packet tables once and keeps one alacgpu_ctx.  A step,
`crops(files, frame_offsets, num_frames)`, is two calls: alacgpu_plan_crops_device (the kernel of csrc/alac_corpus.hip does
`window_plan` for every crop against the resident tables) and alacgpu_decode_window_into_device over the plan it wrote.  The
host hands over (file, first frame) pairs -- or nothing at all when they are device tensors already.

`Corpus.from_pcm` builds the same corpus from PCM that is on the GPU already, without the file system: per batch one
alacgpu_encode_device call into slots, one alacgpu_compact_packets_device call that packs them behind the packets so far (and
writes their offsets), one small read.  `Corpus.save` writes any corpus back as M4A files: its checkpoint.

`Corpus(sources, hbm_bytes=n)` keeps only the first files, as many as fit n bytes, in HBM and the others in page-locked host
memory.  A step is then three calls: between the plan and the decode, alacgpu_stage_packets_device gathers the plan's packets
from both tiers into a small staging blob in HBM, and the decode reads that.

`crops(..., sample_rate=R, mono=)` gives the crops at another rate and as one channel (`Corpus._resampled_crops`): the source
frames a crop needs are decoded as above into a scratch the corpus keeps, and one alacgpu_resample_device call (resample.py
states the filter) resamples every crop out of it.

`crops(..., <a stage keyword>=)` runs stages on the waveform and behind it, in three steps.  `_cropstages._stage_plan` is the
one place that lists the keywords and refuses what a stage cannot take, before any device work, for `crops` and `random_crops`
alike; `_cropstages._middle_draws` makes the draws nobody gave; `Corpus._run` is the one place that lists what runs, in order:
the crops the second corpora make (`Corpus._companion_crops`: the noise of an AddNoise, then the impulse responses of a Reverb,
each cropped by its own corpus at the rate of the crops), the waveform once (`Corpus._waveform`), then every stage that was
asked for by its one library call, in place on the same stream (each stage's module states its arithmetic).

`crops(..., speed=)` plays every crop at a drawn factor in front of all that (the same method, speed.py): the step of a corpus
whose rates differ, with a ratio per (file rate, factor) in place of one per file rate; the crops at factor 1 go through the
table kernels, the others through alacgpu_resample_ratio_rows_device, which evaluates its weights per tap.

`crops(..., pitch=)` changes every crop's pitch by a drawn ratio and keeps its duration, behind the waveform and speed= and in
front of reverb= (pitch.py): alacgpu_time_stretch_device into a scratch, alacgpu_resample_ratio_rows_device into a second one and
alacgpu_copy_rows_device back into the crops, the ratios gathered from the draws on the device.

`Corpus(sources, mixed_rates=True)` takes files of different sample rates.  Crops of such a corpus exist at a target rate only;
a step is the same method and the same launches, with a source window per crop in the plan
(alacgpu_plan_crops_frames_device) and a filter table per row in the resampler (alacgpu_resample_rows_device).

`corpus_tables` (the resident tables as numpy arrays), `entries_per_crop` (the K bound), `stage_bytes_per_crop` (the staging
bound), `tier_split`, `corpus_plan_host`, `compact_plan_host` and `stage_plan_host` (the three kernels' specifications in
numpy) need no device.
"""
import numpy as np

from . import (MAX_FRAME, ST_OK, ST_UNSUPPORTED_ELEMENT, ST_UNSUPPORTED_PREDTYPE, AlacGpuContext, AlacGpuError, PinnedBuffer,
               _Closing, _check, _check_batch_args, _compact_slots, _dp, _encode_slots, _frame_count, _status_text, _torch_dtype,
               _VP, _write_file, lib, make_cfgs)
from ._cropstages import _NEEDS_RATE, _TWO_CHANNELS, _for_batch, _is_f32, _middle_draws, _stage_plan
from .augment import _spec_augment
from .biquad import _biquad
from .level import _level
from .deltas import _add_deltas
from .mix import _mix, snr_ratio
from .normalize import _normalize
from .vad import _select_frames, _vad_energy
from .kaldi_pitch import KaldiPitch, _kaldi_pitch
from .pyin import PYin, _pyin
from .yin import _yin
from .pitch import _pitch_shift, _ratio_kinds
from .reverb import _reverb
from .rir import _simulate
from .speed import MAX_WIDTH as _SPEED_MAX_WIDTH, SpeedPerturb, ratio as _speed_ratio

PAD_CFG = 0xFFFF        # a padding entry's cfg_idx: never a row of the context, so the kernels switch the entry off
MAX_CFGS = 65535


def corpus_tables(tables, mixed_rates=False):
    """The resident tables of a corpus from its files' packet tables (dicts with sizes, durations, cfg, num_channels and
    sample_rate, as container.packet_table returns them; the packet bytes are not looked at).  The packets of all files lie
    back to back.  Returns a dict of numpy arrays: pkt_offset[P] uint64 (into the blob), pkt_size[P] uint32, pkt_end[P] uint64
    (inclusive prefix sum of the durations within the packet's file), file_first[F + 1] uint32, file_cfg[F] uint16 (rows of
    cfgs), cfgs (the distinct alacgpu_cfg rows), num_frames[F] int64, file_base[F + 1] uint64 (where a file's bytes start),
    file_rate[F] int64 (a file's sample rate), and channels, sample_rate, blob_bytes.  ValueError: no files, a file whose
    channel count or sample rate differs from the first's, more than 65535 distinct stream cfgs, 2^32 packets or more.
    mixed_rates: the files may differ in sample rate (not in channel count); sample_rate is then the rate they share, or None
    when they do not share one."""
    from . import CFG_DTYPE

    if not len(tables):
        raise ValueError("no sources")
    channels, rate = int(tables[0]["num_channels"]), int(tables[0]["sample_rate"])
    for i, t in enumerate(tables):
        if int(t["num_channels"]) != channels or (int(t["sample_rate"]) != rate and not mixed_rates):
            raise ValueError(f"source {i}: {t['num_channels']} channels at {t['sample_rate']} Hz, the first has {channels} at {rate} Hz")
    file_rate = np.array([int(t["sample_rate"]) for t in tables], dtype=np.int64)
    if (file_rate != rate).any():
        rate = None
    counts = np.array([len(t["sizes"]) for t in tables], dtype=np.int64)
    if int(counts.sum()) >= 1 << 32:
        raise ValueError(f"{int(counts.sum())} packets: a corpus holds fewer than 2^32")
    file_first = np.zeros(len(tables) + 1, dtype=np.uint32)
    file_first[1:] = np.cumsum(counts)
    sizes = np.concatenate([np.asarray(t["sizes"], dtype=np.uint32) for t in tables])
    ends = np.concatenate([np.cumsum(np.asarray(t["durations"], dtype=np.int64)) for t in tables]).astype(np.uint64)
    pkt_offset = np.zeros(len(sizes), dtype=np.uint64)
    if len(sizes) > 1:
        pkt_offset[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
    blob_bytes = int(sizes.sum(dtype=np.uint64))
    file_base = np.concatenate([pkt_offset, [blob_bytes]]).astype(np.uint64)[file_first]
    rows = np.concatenate([np.ascontiguousarray(t["cfg"], dtype=CFG_DTYPE).reshape(-1)[:1] for t in tables])
    uniq, inverse = np.unique(rows.view(np.uint8).reshape(-1, CFG_DTYPE.itemsize), axis=0, return_inverse=True)
    if len(uniq) > MAX_CFGS:
        raise ValueError(f"{len(uniq)} distinct stream cfgs: a corpus holds at most {MAX_CFGS}")
    num_frames = np.array([int(np.sum(np.asarray(t["durations"], dtype=np.int64))) for t in tables], dtype=np.int64)
    return dict(pkt_offset=pkt_offset, pkt_size=sizes, pkt_end=ends, file_first=file_first,
                file_cfg=np.asarray(inverse).reshape(-1).astype(np.uint16), cfgs=np.ascontiguousarray(uniq).view(CFG_DTYPE).reshape(-1),
                num_frames=num_frames, file_base=file_base, file_rate=file_rate, channels=channels, sample_rate=rate,
                blob_bytes=blob_bytes)


def _widest_windows(pkt_end, file_first, num_frames):
    """The windows of num_frames frames that take the most packets: (g0, g1), two int64 arrays of global packet ranges, among
    which every window's range p0 .. p1 of window_plan is contained in one.  Inside the packet a window starts in, p0 is fixed
    and p1 grows with the offset, so the window from that packet's last frame reaches furthest; a window from frame 0 starts
    at packet 0 whatever the durations.  num_frames: one length, or an array [F] of a length per file (a file's windows are
    then as long as its own entry says; a file with 0 has none)."""
    pkt_end = np.asarray(pkt_end).astype(np.int64)
    file_first = np.asarray(file_first).astype(np.int64)
    F = len(file_first) - 1
    if np.ndim(num_frames) == 0:
        L = np.full(F, int(num_frames), dtype=np.int64)
    else:
        L = np.asarray(num_frames).astype(np.int64).reshape(-1)
        if len(L) != F:
            raise ValueError(f"{len(L)} window lengths for {F} files")
    if not (L > 0).any() or len(pkt_end) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    counts = np.diff(file_first)
    file_of = np.repeat(np.arange(F, dtype=np.int64), counts)
    local = np.arange(len(pkt_end), dtype=np.int64) - file_first[file_of]
    start = np.where(local == 0, 0, np.concatenate([[0], pkt_end[:-1]]))
    total = np.zeros(F, dtype=np.int64)
    total[counts > 0] = pkt_end[file_first[1:][counts > 0] - 1]
    # the candidate windows: from the last frame of every packet that has frames, and from frame 0 of every file
    has = pkt_end > start
    o = np.concatenate([pkt_end[has] - 1, np.zeros(F, dtype=np.int64)])
    f = np.concatenate([file_of[has], np.arange(F, dtype=np.int64)])
    p0 = np.concatenate([local[has], np.zeros(F, dtype=np.int64)])
    p0 = np.where(o == 0, 0, p0)
    keep = L[f] > 0
    o, f, p0 = o[keep], f[keep], p0[keep]
    end = np.minimum(o + L[f], total[f])
    # p1: the file's packets that start in front of `end` -- one search over all files' starts, a file's keyed behind the last's
    M = int(total.max()) + 2
    if F * M < 1 << 62:
        p1 = np.searchsorted(file_of * M + start, f * M + end, side="left") - file_first[f]
    else:
        p1 = np.array([np.searchsorted(start[file_first[k]:file_first[k + 1]], e, side="left") for k, e in zip(f, end)], dtype=np.int64)
    p1 = np.maximum(p1, p0)
    return file_first[f] + p0, file_first[f] + p1


def entries_per_crop(pkt_end, file_first, num_frames):
    """K(L): the most packets a window of num_frames frames takes in any file (the largest p1 - p0 of window_plan over every
    offset), exact: see _widest_windows.  Files of one frame length fl: ceil((L - 1) / fl) + 1 when the file is long enough.
    num_frames may be an array [F]: file f's windows are num_frames[f] frames long (crops at one target rate of files of
    different rates), and K is the most any file's own windows take."""
    g0, g1 = _widest_windows(pkt_end, file_first, num_frames)
    return int((g1 - g0).max()) if len(g0) else 0


def stage_bytes_per_crop(pkt_size, pkt_end, file_first, num_frames):
    """S(L): the most bytes a window of num_frames frames takes in a staging blob, where every packet starts at a multiple of
    16 -- the largest sum of the sizes, each rounded up to 16, over the packets p0 .. p1 of window_plan over every offset of
    every file, exact (some offset reaches it; see _widest_windows: the widest windows contain every other window's packets).
    Never more than the largest such sum over K(L) consecutive packets of one file, and equal to it where one file both takes
    K(L) packets and has the largest ones.  B crops never stage more than B * S(L) bytes.  num_frames may be an array [F] of a
    window length per file, as for entries_per_crop."""
    g0, g1 = _widest_windows(pkt_end, file_first, num_frames)
    if not len(g0):
        return 0
    rounded = (np.asarray(pkt_size).astype(np.int64) + 15) // 16 * 16
    run = np.concatenate([[0], np.cumsum(rounded)])
    return int((run[g1] - run[g0]).max())


def tier_split(file_bytes, hbm_bytes):
    """How many of a corpus's files go to the device blob: the longest prefix of the files (in order; file_bytes[f]: the packet
    bytes of file f) whose bytes together fit hbm_bytes; every file behind it goes to the host blob, so a file is never
    split.  None: all of them.  ValueError: hbm_bytes negative or not an integer."""
    file_bytes = np.asarray(file_bytes).astype(np.int64)
    if hbm_bytes is None:
        return len(file_bytes)
    if isinstance(hbm_bytes, (bool, np.bool_)) or not isinstance(hbm_bytes, (int, np.integer)) or int(hbm_bytes) < 0:
        raise ValueError(f"hbm_bytes must be None or a non-negative integer, not {hbm_bytes!r}")
    return int(np.searchsorted(np.cumsum(file_bytes), int(hbm_bytes), side="right"))


def corpus_plan_host(pkt_offset, pkt_size, pkt_end, file_first, file_cfg, crop_file, crop_offset, num_frames, entries, dst_stride,
                     crop_frames=None):
    """alacgpu_plan_crops_device on the host, in numpy: the kernel's specification (tests compare the two; `Corpus.crops` never
    comes here).  Returns (offsets uint64, sizes uint32, cfg_idx uint16, dst_first uint64, dst_frames uint32, src_skip uint32)
    of B * entries entries, crop-major, and lengths[B] int64: min(num_frames, T_f - offset); -1 for a file index >= F or an
    offset > T_f; -2 for a crop that needs more than `entries` entries.  Entries behind a crop's packets are padding:
    cfg_idx 0xFFFF and zeros.  crop_frames: alacgpu_plan_crops_frames_device -- a window length per crop [B] (uint32) with
    num_frames as their bound: lengths[b] = min(crop_frames[b], T_f - offset), and -1 with padding only for a crop_frames[b]
    above num_frames."""
    pkt_offset, pkt_size = np.asarray(pkt_offset, dtype=np.uint64), np.asarray(pkt_size, dtype=np.uint32)
    ends_all = np.asarray(pkt_end).astype(np.int64)
    file_first, file_cfg = np.asarray(file_first).astype(np.int64), np.asarray(file_cfg, dtype=np.uint16)
    crop_file, crop_offset = np.asarray(crop_file, dtype=np.uint32), np.asarray(crop_offset, dtype=np.uint64)
    B, K, L, F = len(crop_file), int(entries), int(num_frames), len(file_first) - 1
    offsets, sizes = np.zeros(B * K, np.uint64), np.zeros(B * K, np.uint32)
    cfg_idx = np.full(B * K, PAD_CFG, np.uint16)
    dst_first, dst_frames, src_skip = np.zeros(B * K, np.uint64), np.zeros(B * K, np.uint32), np.zeros(B * K, np.uint32)
    lengths = np.full(B, -1, np.int64)
    each = None if crop_frames is None else np.asarray(crop_frames, dtype=np.uint32)
    if each is not None and each.shape != (B,):
        raise ValueError(f"{each.shape} window lengths for {B} crops")
    bound = L
    for b in range(B):
        f, o = int(crop_file[b]), int(crop_offset[b])
        if each is not None:
            L = int(each[b])
        if f >= F or L > bound:
            continue
        g0, g1 = int(file_first[f]), int(file_first[f + 1])
        ends = ends_all[g0:g1]
        total = int(ends[-1]) if g1 > g0 else 0
        if o > total:
            continue
        length = min(L, total - o)
        lengths[b] = length
        if length == 0 or g1 == g0:
            continue
        end = o + length
        starts = np.concatenate([[0], ends[:-1]])
        p0 = 0 if o == 0 else int(np.searchsorted(ends, o, side="right"))       # the first packet that ends past o
        p1 = max(int(np.searchsorted(starts, end, side="left")), p0)            # packets that start in front of the end
        if p1 - p0 > K:
            lengths[b] = -2
            continue
        j = slice(b * K, b * K + p1 - p0)
        lo = np.maximum(starts[p0:p1], o)
        offsets[j], sizes[j], cfg_idx[j] = pkt_offset[g0 + p0:g0 + p1], pkt_size[g0 + p0:g0 + p1], file_cfg[f]
        dst_first[j] = (b * int(dst_stride) + (lo - o)).astype(np.uint64)
        dst_frames[j] = np.maximum(np.minimum(ends[p0:p1], end) - lo, 0)
        src_skip[j] = np.minimum(lo - starts[p0:p1], MAX_FRAME)
    return offsets, sizes, cfg_idx, dst_first, dst_frames, src_skip, lengths


def compact_plan_host(sizes, slot_bytes, base, capacity):
    """alacgpu_compact_packets_device on the host, in numpy: the kernel's specification (tests compare the two; the product
    never comes here).  Returns (pkt_offset uint64 [n]: base + the counted sizes in front of a packet -- a size above
    slot_bytes counts as 0 --, total: the sum of the counted sizes whatever the capacity, copied bool [n]: the packets with
    pkt_offset + size <= capacity -- those, whole, are all that is written to the blob)."""
    sizes = np.asarray(sizes, dtype=np.uint32).astype(np.uint64)
    counted = np.where(sizes <= np.uint64(slot_bytes), sizes, np.uint64(0))
    ends = np.cumsum(counted, dtype=np.uint64)
    pkt_offset = np.uint64(base) + ends - counted
    total = int(ends[-1]) if len(ends) else 0
    copied = pkt_offset.astype(object) + counted.astype(object) <= int(capacity) if len(ends) else np.zeros(0, dtype=bool)
    return pkt_offset.astype(np.uint64), total, np.asarray(copied, dtype=bool)


def stage_plan_host(src_offset, sizes, lo_bytes, hi_bytes, capacity):
    """alacgpu_stage_packets_device on the host, in numpy: the kernel's specification (tests compare the two; the product
    never comes here).  The source space is lo_bytes of one part and hi_bytes of another behind it; a packet counts with its
    size when it lies wholly inside one part, else as 0.  Returns (stage_offset uint64 [n]: the counted sizes in front of a
    packet, each rounded up to 16, total: that sum over all packets whatever the capacity, copied bool [n]: the packets with
    a counted size above 0 and stage_offset + the rounded size <= capacity -- those, whole, are all that is copied)."""
    off = [int(x) for x in np.asarray(src_offset, dtype=np.uint64)]
    size = [int(x) for x in np.asarray(sizes, dtype=np.uint32)]
    lo, hi = int(lo_bytes), int(hi_bytes)
    inside = [(o < lo and o + n <= lo) or (o >= lo and o + n <= lo + hi) for o, n in zip(off, size)]
    rounded = np.array([(n + 15) // 16 * 16 if ok else 0 for n, ok in zip(size, inside)], dtype=np.uint64).reshape(-1)
    ends = np.cumsum(rounded, dtype=np.uint64)
    stage_offset = ends - rounded
    total = int(ends[-1]) if len(ends) else 0
    copied = np.array([r > 0 and int(e) <= int(capacity) for r, e in zip(rounded, ends)], dtype=bool).reshape(-1)
    return stage_offset.astype(np.uint64), total, copied


class Corpus(_Closing):
    """M4A files resident in HBM, compressed: Corpus(sources, device=0) demuxes every source once (file bytes, a path or a
    seekable binary file object, as for `load`), uploads the packet bytes file by file into one device blob and the packet
    tables next to it, and keeps one alacgpu_ctx until close().  All files share channel count and sample rate (ValueError
    naming the first that differs); 16- and 24-bit may mix; files that share a stream cfg share its row (at most 65535
    distinct ones).  num_files, num_frames (int64 host array [F]), channels, sample_rate.  Calls on one Corpus belong on one
    stream: the plan arrays are reused from call to call.

    hbm_bytes: None keeps every file in HBM.  An integer keeps the longest prefix of the files whose packet bytes fit that
    many bytes in HBM and every file behind it in one page-locked host blob (`tier_split`; a file is never split, 0 puts all
    of them on the host; ValueError when negative or not an integer); tier_bytes is (device bytes, host bytes).  Crops of
    such a corpus are what they are of the resident one, bit for bit: a step additionally gathers the packets it needs from
    both tiers into a staging blob in HBM (alacgpu_stage_packets_device; at most batch * stage_bytes_per_crop(num_frames)
    bytes, kept and reused), and the decode reads that.  When every file fits, the corpus is the resident one.

    mixed_rates=True: the files may differ in sample rate (not in channel count).  sample_rates (int64 host array [F]) has
    every file's; sample_rate is the one they share, or None when they differ.  num_frames stays in source frames.  Crops of
    a corpus whose rates differ exist at a target rate only: crops / random_crops want sample_rate=R (`_resampled_crops`), and
    every file is resampled by its own ratio in the same launches.  Files that happen to share one rate make the corpus
    Corpus(sources) is, call for call."""

    def __init__(self, sources, device=0, hbm_bytes=None, mixed_rates=False):
        import torch

        from .container import header_table, packet_table

        self._gpu = self._pinned = None
        sources = list(sources)
        # the headers first (no packet bytes): the blobs' sizes; a file object is read twice from where it stands
        where = [s.tell() if hasattr(s, "tell") and hasattr(s, "seek") else None for s in sources]
        file_bytes = []
        for s, pos in zip(sources, where):
            file_bytes.append(int(header_table(s)["sizes"].sum(dtype=np.int64)))
            if pos is not None:
                s.seek(pos)
        on_device = tier_split(file_bytes, hbm_bytes)
        total, lo_bytes = sum(file_bytes), sum(file_bytes[:on_device])
        dev = torch.device("cuda", device)
        # readable up to blob_bytes rounded up to 16, as every decode entry point wants it (torch's allocations are aligned)
        self._blob = torch.zeros(lo_bytes + 64, dtype=torch.uint8, device=dev)
        try:
            if total > lo_bytes:
                with torch.cuda.device(dev):
                    self._pinned = PinnedBuffer(total - lo_bytes + 64, np.uint8)
                self._pinned.array[total - lo_bytes:] = 0
            heads, base = [], 0
            for f, s in enumerate(sources):
                t = packet_table(s)
                n = int(t["sizes"].sum(dtype=np.int64))
                if n and f < on_device:
                    self._blob[base:base + n].copy_(torch.from_numpy(np.array(t["blob"][:n])))
                elif n:
                    if base - lo_bytes + n > total - lo_bytes:
                        raise ValueError("a source changed while it was read")
                    self._pinned.array[base - lo_bytes:base - lo_bytes + n] = t["blob"][:n]
                base += n
                if f + 1 == on_device and base != lo_bytes:
                    raise ValueError("a source changed while it was read")
                heads.append({k: t[k] for k in ("sizes", "durations", "cfg", "num_channels", "sample_rate")})
            if base != total:
                raise ValueError("a source changed while it was read")
            self._install(device, corpus_tables(heads, mixed_rates=mixed_rates), host_bytes=total - lo_bytes)
        except BaseException:
            self._free_pinned()
            raise

    def _free_pinned(self):
        if getattr(self, "_pinned", None) is not None:
            self._pinned.close()
            self._pinned = None

    def _install(self, device, tb, d_pkt_offset=None, d_pkt_size=None, gpu=None, host_bytes=0):
        """The end of both constructors: self._blob holds the packets; tb: the host tables (pkt_end, file_first, file_cfg, cfgs,
        num_frames, channels, sample_rate, blob_bytes, and pkt_offset and pkt_size unless they are on the device already: the
        two tensors; `save` fetches them then); gpu: the context to keep, if there is one already."""
        import torch

        dev = self._dev = torch.device("cuda", device)
        self.device = device

        def up(a, dtype):      # (an empty table still needs an address)
            a = np.ascontiguousarray(a).view(dtype)
            return torch.from_numpy(a if len(a) else np.zeros(1, dtype)).to(dev)

        self.num_files = len(tb["file_cfg"])
        self.num_frames = tb["num_frames"]
        self.channels, self.sample_rate = tb["channels"], tb["sample_rate"]
        self.sample_rates = np.asarray(tb["file_rate"] if "file_rate" in tb else np.full(self.num_files, tb["sample_rate"]), dtype=np.int64)
        self._host = tb
        self._blob_bytes = tb["blob_bytes"]
        self._pkt_offset = d_pkt_offset if d_pkt_offset is not None else up(tb["pkt_offset"], np.int64)
        self._pkt_size = d_pkt_size if d_pkt_size is not None else up(tb["pkt_size"], np.int32)
        self._pkt_end, self._file_first = up(tb["pkt_end"], np.int64), up(tb["file_first"], np.int32)
        self._file_cfg = up(tb["file_cfg"], np.int16)
        self._d_num_frames = torch.from_numpy(self.num_frames).to(dev)
        self._plan, self._capacity, self._last = None, 0, 0
        # the tiers: the first bytes of the packets' address space are self._blob's, the others the page-locked blob's
        self._pinned = getattr(self, "_pinned", None)
        self._hi_bytes = int(host_bytes)
        self._lo_bytes = self._blob_bytes - self._hi_bytes
        self._stage = self._stage_plan = None
        self._stage_room, self._stage_entries, self._stage_bytes = 0, 0, 0
        self._rs_scratch = None                           # crops at another rate: the decoded source crops
        self._ft_scratch = None                           # crops(features=): the crops the feature kernel reads
        self._delta_scratch = None                        # crops(deltas=): the features the delta kernel reads
        self._vad_scratch = None                          # crops(vad=): the decisions between the VAD and the selection
        self._f0_scratch = None                           # crops(f0=): the F0 track the call returns
        self._mix_scratch = None                          # crops(mix=): the noise crops, whichever corpus makes them
        self._reverb_scratch = None                       # crops(reverb=): the impulse responses of the crops
        self._pitch_scratch = None                        # crops(pitch=): the stretched rows
        self._pitch_back_scratch = None                   # ... and those rows resampled, in front of their copy into the crops
        self._rates, self._windows = {}, {}               # `_rate` per (target rate, factors); `_window` per (rate or None, L, factors)
        self._gpu = gpu if gpu is not None else AlacGpuContext(tb["cfgs"], device)

    @classmethod
    def from_pcm(cls, pcm, lengths=None, sample_rate=None, sample_size=16, frame_length=4096):
        """The corpus of PCM that is on the GPU, without files in between: from_pcm(pcm, lengths, sample_rate, sample_size=16,
        frame_length=4096) -- exactly `save_batch`'s arguments and checks (file f is frames 0 .. lengths[f] of pcm[f],
        [F, C, Tmax] int32 or float32) -- or from_pcm(batches, sample_rate=...) with an iterable of (pcm, lengths) pairs, taken
        one after the other so that the PCM never has to exist all at once; every batch has the same channel count, F and
        Tmax may differ.  Files are numbered in the order given; the device is the tensors'.  Per batch: one encode into
        slots, one compaction behind the packets so far, one small read; the blob grows geometrically where a batch does
        not fit (build_stats: batches, compactions, grown, capacity).  The corpus is byte for byte the one
        Corpus(the files save_batch writes) is.  ValueError before a batch's device work as for save_batch; "no sources"
        for an empty iterable; AlacGpuError naming file and packet for a packet that was not encoded."""
        import torch

        single = isinstance(pcm, torch.Tensor) or lengths is not None
        batches = [(pcm, lengths)] if single else pcm
        self = cls.__new__(cls)
        self._gpu = None
        gpu = dev = None
        blob, cap, base = None, 0, 0
        stats = dict(batches=0, compactions=0, grown=0, capacity=0)
        offs, sizes, ends, counts, frames_of = [], [], [], [], []
        try:
            for x, lens in batches:
                F, C_, T, lens = _check_batch_args(x, lens, sample_rate, sample_size, frame_length)
                fl = int(frame_length)
                if gpu is None:
                    dev, channels = x.device, C_
                    row = make_cfgs([(fl, sample_size, 40, 10, 14, C_)])
                    row["ctor_sample_size"] = sample_size      # (as the file's cookie and sample entry give it)
                    gpu = AlacGpuContext(row, dev.index if dev.index is not None else torch.cuda.current_device())
                elif C_ != channels or x.device != dev:
                    raise ValueError(f"batch {stats['batches']}: {C_} channels on {x.device}, the first has {channels} on {dev}")
                with torch.cuda.device(dev):
                    stream = torch.cuda.current_stream(dev).cuda_stream
                    e = _encode_slots(gpu, x, lens, fl, stream)
                    if sum(counts) + e.n >= 1 << 32:
                        raise ValueError("a corpus holds fewer than 2^32 packets")
                    if blob is None:    # the first guess: three quarters of the samples' bytes (cfg2-shaped audio takes two thirds)
                        cap = max(sum(lens) * C_ * (sample_size // 8) * 3 // 4, 4096)
                        blob = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
                    d_off = torch.empty(e.n, dtype=torch.int64, device=dev)
                    while True:
                        total, bad = _compact_slots(gpu, e, blob, base, cap, d_off, stream)
                        stats["compactions"] += 1
                        if bad < e.n:
                            f, q = int(e.file_of[bad]), bad - int(np.sum(e.counts[:int(e.file_of[bad])]))
                            raise AlacGpuError(f"file {len(counts) + f}, packet {q} was not encoded: {_status_text(int(e.d_st[bad]))}")
                        if base + total <= cap:
                            break
                        # it did not fit: a larger blob, what is there copied over, and the compaction alone again
                        cap = max(base + total, cap + cap // 2)
                        old, blob = blob, None
                        if base == 0:
                            old = None                           # (nothing to keep: the old one goes first)
                        blob = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
                        if old is not None:
                            blob[:base].copy_(old[:base])
                        old = None
                        stats["grown"] += 1
                    base += total
                    offs.append(d_off)
                    sizes.append(e.d_sizes)
                    counts += e.counts
                    ends += [np.cumsum(e.frames[e.file_of == f]) for f in range(F)]
                    frames_of += lens
                    stats["batches"] += 1
                    e = None                                     # the slot buffer goes before the next batch is encoded
            if gpu is None:
                raise ValueError("no sources")
        except BaseException:
            if gpu is not None:
                gpu.close()
            raise
        blob[base:base + 64].zero_()      # (a compaction that did not fit may have left packets behind the last one)
        stats["capacity"] = cap
        file_first = np.zeros(len(counts) + 1, dtype=np.uint32)
        file_first[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
        tb = dict(pkt_end=np.concatenate(ends).astype(np.uint64), file_first=file_first,
                  file_cfg=np.zeros(len(counts), dtype=np.uint16), cfgs=gpu.cfgs, num_frames=np.asarray(frames_of, dtype=np.int64),
                  channels=channels, sample_rate=int(sample_rate), blob_bytes=base)
        self._blob = blob
        self.build_stats = stats
        self._install(gpu.device, tb, torch.cat(offs) if len(offs) > 1 else offs[0], torch.cat(sizes) if len(sizes) > 1 else sizes[0], gpu)
        return self

    def _host_table(self, name):
        """pkt_offset / pkt_size on the host: a corpus from PCM has them on the device only until somebody asks."""
        if name not in self._host:
            dtype = np.uint64 if name == "pkt_offset" else np.uint32
            d = self._pkt_offset if name == "pkt_offset" else self._pkt_size
            self._host[name] = d.cpu().numpy().view(dtype)[:len(self._host["pkt_end"])]
        return self._host[name]

    def save(self, dests, sample_rate=None):
        """Write file f of the corpus as an M4A file to dests[f] (paths or writable binary file objects; sample_rate: the
        file's own unless given): the checkpoint of a corpus -- Corpus(those files) is the same corpus again, and for a corpus
        from_pcm made the files are byte for byte what save_batch writes for the same arguments.  A packet's duration is the
        difference of its pkt_end to the one in front; frame length, sample size and the Rice parameters are the file's cfg
        row's.  The packets cross to the host file by file.  Returns the file sizes."""
        self._open()
        dests = list(dests)
        if len(dests) != self.num_files:
            raise ValueError(f"{self.num_files} files in the corpus and {len(dests)} destinations")
        if sample_rate is not None and (not isinstance(sample_rate, (int, np.integer)) or not 1 <= int(sample_rate) < 1 << 32):
            raise ValueError(f"sample_rate must be a positive 32-bit integer, not {sample_rate}")
        h = self._host
        off, size = self._host_table("pkt_offset").astype(np.int64), self._host_table("pkt_size").astype(np.int64)
        out = []
        for f, dest in enumerate(dests):
            g0, g1 = int(h["file_first"][f]), int(h["file_first"][f + 1])
            if g1 == g0:
                raise ValueError(f"file {f} has no packets: nothing to write")
            lo, hi = int(off[g0]), int(off[g1 - 1] + size[g1 - 1])
            if self._hi_bytes and lo >= self._lo_bytes:       # a file of the host tier: straight from the host blob
                data = self._pinned.array[lo - self._lo_bytes:hi - self._lo_bytes].tobytes()
            else:
                data = self._blob[lo:hi].cpu().numpy().tobytes()
            packets = [data[int(off[g]) - lo:int(off[g]) - lo + int(size[g])] for g in range(g0, g1)]
            ends = h["pkt_end"][g0:g1].astype(np.int64)
            durations = np.diff(np.concatenate([[0], ends]))
            c = h["cfgs"][int(h["file_cfg"][f])]
            rate = self.sample_rates[f] if sample_rate is None else sample_rate
            out.append(_write_file(dest, packets, durations, int(c["max_samples_per_frame"]), int(c["sample_size"]), self.channels,
                                   int(rate), rice=(int(c["rice_history_mult"]), int(c["rice_initial_history"]), int(c["rice_kmodifier"]))))
        return out

    def _open(self):
        if self._gpu is None:
            raise AlacGpuError("the corpus is closed")

    def close(self):
        if getattr(self, "_gpu", None) is not None:
            self._gpu.close()
            self._gpu = None
            self._blob = self._plan = self._stage = self._stage_plan = self._rs_scratch = self._ft_scratch = self._delta_scratch = self._vad_scratch = self._f0_scratch = self._mix_scratch = self._reverb_scratch = self._pitch_scratch = self._pitch_back_scratch = None
        self._free_pinned()

    @property
    def tier_bytes(self):
        """(device_bytes, host_bytes): the packet bytes in HBM and those in page-locked host memory"""
        return self._lo_bytes, self._hi_bytes

    def stage_bytes_per_crop(self, num_frames, sample_rate=None):
        """S for crops of num_frames frames: the bytes the staging blob reserves per crop (computed once per length).
        sample_rate, for a corpus whose rates differ: S of the crops of num_frames frames at that rate -- a file counts with
        the source window its own ratio needs."""
        win = self._window_of(num_frames, sample_rate)
        if win["S"] is None:        # (no host tier: no step has needed it)
            win["S"] = stage_bytes_per_crop(self._host_table("pkt_size"), self._host["pkt_end"], self._host["file_first"], win["Ls"])
        return win["S"]

    def _stage_arrays(self, n, room):
        """The staging blob (room bytes and 64 more: readable past blob_bytes, as the resident blob is) and the staged offsets
        of n entries, kept and reused while neither grows."""
        import torch

        room = max(room, 16)        # (a step whose packets are all empty still hands the library a blob)
        if room > self._stage_room:
            self._stage = None      # (the old one goes first)
            self._stage = torch.zeros(room + 64, dtype=torch.uint8, device=self._dev)
            self._stage_room = room
        if n > self._stage_entries:
            self._stage_plan = None
            self._stage_plan = dict(offsets=torch.empty(n, dtype=torch.int64, device=self._dev),
                                    total=torch.zeros(1, dtype=torch.int64, device=self._dev))
            self._stage_entries = n
        return self._stage, self._stage_plan

    def entries_per_crop(self, num_frames, sample_rate=None):
        """K for crops of num_frames frames: the entries the plan reserves per crop (computed once per length).  sample_rate,
        for a corpus whose rates differ: K of the crops of num_frames frames at that rate, as for stage_bytes_per_crop."""
        return self._window_of(num_frames, sample_rate)["K"]

    def _window_of(self, num_frames, sample_rate):
        """The window behind the public K and S: a corpus that has a rate of its own ignores sample_rate"""
        if sample_rate is not None and self.sample_rate is None:
            return self._window(sample_rate, _frame_count("num_frames", num_frames))
        return self._window(None, int(num_frames))

    def _window(self, R, L, speed=None):
        """Per (target rate, crop length, factors), once: Ls, the source frames a crop's window takes -- L itself for R None,
        the native window; else resample.source_window's bound by `_rate(R, speed)`: an int, or for its per-crop variant
        int64 [F], a file's largest window over the factors (speed: a SpeedPerturb; None: the one factor 1), and then d_Ls as
        well, int32 [kinds] on the device, the window of every kind --, Ls_max, the largest, and K and S, where a file counts
        with its own Ls.  S only where there is a host tier, else None: the packet sizes of a corpus from PCM would have to
        come from the device for it."""
        import torch

        key = (R, L, None if speed is None else speed.factors)
        if key not in self._windows:
            Ls = each = L
            if R is not None:
                rt = self._rate(R, speed)
                each = ((max(L, 1) - 1) // rt["b"] + 2) * rt["a"] + 2 * rt["width"]
                Ls = each.reshape(-1, rt["nk"]).max(axis=1)[rt["rate_of"]] if np.ndim(each) else each
                if int(np.max(Ls)) >= 1 << 32:
                    raise ValueError(f"num_frames {L} needs {int(np.max(Ls))} source frames: that does not fit 32 bits")
            h = self._host
            win = dict(Ls=Ls, Ls_max=int(np.max(Ls)), K=max(entries_per_crop(h["pkt_end"], h["file_first"], Ls), 1),
                       S=stage_bytes_per_crop(self._host_table("pkt_size"), h["pkt_end"], h["file_first"], Ls) if self._hi_bytes else None)
            if np.ndim(each):
                win["d_Ls"] = torch.from_numpy(each.astype(np.uint32).view(np.int32)).to(self._dev)
            self._windows[key] = win
        return self._windows[key]

    def _plan_arrays(self, n):
        """The six plan arrays and the status array, kept and reused while n does not grow past them."""
        import torch

        if n > self._capacity:
            dev, cap = self._dev, n
            self._plan = None       # (the old ones go first)
            self._plan = dict(offsets=torch.empty(cap, dtype=torch.int64, device=dev), sizes=torch.empty(cap, dtype=torch.int32, device=dev),
                              cfg_idx=torch.empty(cap, dtype=torch.int16, device=dev), dst_first=torch.empty(cap, dtype=torch.int64, device=dev),
                              dst_frames=torch.empty(cap, dtype=torch.int32, device=dev), src_skip=torch.empty(cap, dtype=torch.int32, device=dev),
                              status=torch.empty(cap, dtype=torch.int32, device=dev), iota=torch.arange(cap, dtype=torch.int64, device=dev))
            self._capacity = cap
        return self._plan

    def _indices(self, files, frame_offsets, totals=None):
        """The crops' (file, first frame) as device tensors (int32 / int64: the kernel reads them as unsigned) and whether they
        came from the host (and are checked here) or were device tensors already (and are checked by the kernel).  totals: the
        files' frame counts the offsets are checked against (default num_frames)."""
        import torch

        totals = self.num_frames if totals is None else totals

        on_device = [isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in (files, frame_offsets)]
        if all(on_device):
            if files.dim() != 1 or frame_offsets.dim() != 1 or files.shape != frame_offsets.shape:
                raise ValueError(f"files {tuple(files.shape)} and frame_offsets {tuple(frame_offsets.shape)} must be two vectors of one length")
            if files.dtype.is_floating_point or frame_offsets.dtype.is_floating_point:
                raise ValueError("files and frame_offsets must be integer tensors")
            f = files if files.dtype == torch.int32 else files.clamp(-1, (1 << 31) - 1).to(torch.int32)
            return f.to(self._dev).contiguous(), frame_offsets.to(self._dev, torch.int64).contiguous(), False
        as_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        f, o = as_np(files), as_np(frame_offsets)
        if f.ndim != 1 or o.ndim != 1 or len(f) != len(o):
            raise ValueError(f"{f.shape} files and {o.shape} frame offsets: two sequences of one length")
        if len(f) and (f.dtype.kind not in "iu" or o.dtype.kind not in "iu"):
            raise ValueError("files and frame_offsets must be integers")
        f, o = f.astype(np.int64), o.astype(np.int64)
        bad = np.nonzero((f < 0) | (f >= self.num_files))[0]
        if len(bad):
            raise ValueError(f"crop {int(bad[0])}: file {int(f[bad[0]])} outside 0 .. {self.num_files - 1}")
        bad = np.nonzero((o < 0) | (o > totals[f]))[0]
        if len(bad):
            b = int(bad[0])
            raise ValueError(f"crop {b} (source {int(f[b])}): frame offset {int(o[b])} outside 0 .. {int(totals[f[b]])}")
        return torch.from_numpy(f.astype(np.int32)).to(self._dev), torch.from_numpy(o).to(self._dev), True

    def crops(self, files, frame_offsets, num_frames, dtype=None, out=None, check=True, features=None, normalize=None, mix=None,
              reverb=None, speed=None, pitch=None, f0=None, effects=None, level=None, deltas=None, vad=None, augment=None, sample_rate=None,
              mono=False):
        """Decode crop b = frames frame_offsets[b] .. + num_frames of file files[b] for every b in ONE launch pair: returns
        (pcm [B, C, num_frames] on the device, zero behind lengths[b]; lengths [B], a DEVICE int64 tensor: min(num_frames,
        T_f - offset)).  float32 (default) or int32, as `load`.  files / frame_offsets: sequences, numpy arrays or torch
        tensors.  Tensors already on the device are used as they are -- no copy to the host, no synchronisation; a file index
        or an offset outside the corpus then gives lengths[b] = -1 and a row of zeros.  Anything else is checked on the host
        (ValueError before any device work) and uploaded.  out: a contiguous device tensor of that shape and dtype to decode
        into (it is zeroed first).  check=True reads one small result back: AlacGpuError naming crop, source and packet (its
        index in its file) for the first packet that does not decode (statuses read as `load_batch` reads them), ValueError for
        the first crop with a negative length.  check=False reads nothing back and returns behind the enqueue: see
        last_status().

        sample_rate / mono: crops at another rate and as one channel (`_resampled_crops`): frame_offsets and num_frames then
        count frames at sample_rate, pcm is float32 [B, 1 if mono else C, num_frames].  The defaults -- and the corpus's own
        rate, and mono of one channel -- are the path above.  A corpus whose files differ in rate (mixed_rates=True) has no
        rate of its own: sample_rate is required (ValueError without), and every crop comes through it.

        speed: speed perturbation of the waveform, in front of everything else: a speed.SpeedPerturb, whose draws are then made
        here from the device's default generator, or the pair (SpeedPerturb, draws) with the int64 tensor [B] that its
        `draw(B)` returned.  Crop b is then frames frame_offsets[b] .. + num_frames of its file PLAYED AT ITS FACTOR and
        resampled as a whole to the rate of the crops (`_resampled_crops`); a crop that draws factor 1 is bit for bit the crop of
        the call without speed=.  Every stage behind it sees the perturbed waveform.  ValueError: int32 crops, a corpus of
        more than 2 channels, draws that are not an integer tensor [B] on the corpus's device.

        pitch: pitch shift of the waveform with the duration kept, behind speed= and in front of every other stage -- the
        source's pitch changes, not the room's: a pitch.PitchShift, whose draws are then made here from the device's default
        generator (in front of an AddNoise's), or the pair (PitchShift, draws) with the int64 tensor [B] that its `draw(B)`
        returned.  Bit for bit pitch.pitch_shift(the crops without it, the drawn ratios, rate of the crops, lengths,
        pitch.n_fft): a crop that draws the ratio 1, one of at most n_fft / 2 valid frames and one outside the corpus stay as
        they are; lengths stay.  The stretched rows live in two scratches the corpus keeps.  ValueError: int32 crops, crops
        without a rate, more than 2 channels, something that is no PitchShift, draws that are not an integer tensor [B] on the
        corpus's device, num_frames of at most n_fft / 2.  Tempo perturbation is not a stage here: it changes the source window,
        as speed= does; pitch.time_stretch on the result covers it.

        The stages behind the waveform go by keyword, as sample_rate and mono do, and run in this order whichever are
        given -- pitch, reverb, mix, level, effects, f0, features, deltas, the VAD's decision, normalize, the selection of the
        voiced frames, augment --, in place but for the features and the deltas, by the corpus's own context on the same
        stream; lengths (but for vad=, which shortens them), `check` and last_status() are those of the call without them
        (with check=True a second corpus's own check runs too, and first).  ValueError before any device work for what a
        stage cannot take (`_cropstages._stage_plan`, which `random_crops` runs in front of its first draw).

        reverb: room reverberation of the waveform: a reverb.Reverb, whose draws are then made here from the device's default
        generator, or the pair (Reverb, draws) with the draws that its `draw(B)` returned.  Bit for bit reverb.reverb(the crops
        without it, the first Reverb.frames(rate) frames of the drawn responses at the rate of the crops, lengths, their
        lengths, 0 where a crop drew none).  A Reverb over a rir.ShoeboxRooms: the responses are rir.simulate_rir(geometry,
        beta of the draws, rate, Reverb.frames(rate)) instead, one channel, their lengths 0 where a room is refused.

        mix: noise from a second corpus into the waveform: a mix.AddNoise, whose draws are then made here from the device's
        default generator (in front of a Reverb's), or the pair (AddNoise, draws) with the draws that its `draw(B, num_frames,
        rate of the crops)` returned.  Bit for bit mix.mix(the crops without it, the noise crops, snr_db, lengths, their
        lengths).  The noise and the responses are cropped by their own corpus's `crops` at the rate of the crops, as one
        channel when its channel count is not theirs, into scratches THIS corpus keeps: a second corpus may be this one.

        level: a level.Level -- every crop brought to a peak, an RMS level or a BS.1770 loudness over its valid frames, behind
        the noise and in front of the effects, so that a random gain perturbs around the target.  Bit for bit
        level.level(the crops without it, level, rate of the crops, lengths); a crop outside the corpus stays zeros, and so does
        a silent one.  It draws nothing.  ValueError: int32 crops, something that is no Level, and for lufs more than 5
        channels, crops without a rate, a rate below 160 Hz or not above 3000 Hz.

        effects: the channel, last on the waveform: a biquad.Effects -- a cascade of biquad sections and a gain per crop --,
        whose draws are then made here from the device's default generator (behind a Reverb's and in front of a SpecAugment's --
        and in front of a SpeedPerturb's, which `crops` draws with the waveform; `random_crops` draws the speed first),
        or the pair (Effects, draws) with the (coeffs float64 [B, S, 5], gain float64 [B]) that its `draw(B, rate of the
        crops)` returned.  Bit for bit biquad.biquad(the crops without it, coeffs, lengths, gain, effects.clamp); a crop
        outside the corpus stays zeros.  ValueError: int32 crops, draws of another shape, dtype or device, a filter frequency at
        or above the Nyquist frequency of the crops' rate.

        f0: a yin.Yin -- the F0 track of the final waveform, the one behind speed=, pitch=, reverb=, mix=, level= and effects=
        that features= reads: ONE alacgpu_yin_device call.  The result then gains one element at its end: (pcm or feats,
        lengths, track), track float32 [B, 1 if mono else C, 2, f0.frames(num_frames)] -- f0 in Hz and the aperiodicity,
        yin.py states them --, cut from a scratch the corpus keeps: the next call with f0= writes it again.  Bit for bit
        yin.yin(the waveform the call returns with the same arguments and draws and without features=, f0, lengths); a crop
        outside the corpus is silence.  `Yin.like(features)` has the frames of the features.  ValueError: something that is no
        Yin, a Yin for another rate than the crops', int32 crops, vad= (the selected frames would no longer line up with the
        track), num_frames below f0.min_frames.  Or a pyin.PYin, wherever a Yin is taken and with the same refusals: the
        smoothed track of probabilistic YIN, ONE alacgpu_pyin_device call (two launches), track float32 [B, 1 if mono else C,
        3, f0.frames(num_frames)] -- the decoded bin's frequency in Hz, 1.0 where voiced, the voicing probability, pyin.py
        states them --, bit for bit pyin.pyin of that waveform.  Or a kaldi_pitch.KaldiPitch, again with the same refusals:
        Kaldi's pitch features, ONE alacgpu_kaldi_pitch_device call (three launches), track float32 [B, 1 if mono else C,
        f0.lines, f0.frames(num_frames)] -- kaldi_pitch.py states the lines --, bit for bit kaldi_pitch.kaldi_pitch of that
        waveform; with features=spec and f0=KaldiPitch.like(spec), torch.cat([feats, track], 2) is the pasted matrix.

        features: a features.LogMel, a fbank.KaldiFbank, a mfcc.KaldiMfcc, a cqt.ConstantQ or a stft.Spectrogram -- the crops' log-mel, Kaldi fbank, Kaldi MFCC,
        constant-Q features or spectrogram instead of their PCM (n_mels below is then the transform's line count: a KaldiMfcc's n_ceps, a ConstantQ's n_bins,
        a Spectrogram's bins, filterbank rows or, for the complex spectrum, twice its bins -- that kind takes no deltas=, normalize=, vad= or augment=):
        the waveform goes into a float32 scratch the corpus keeps and ONE alacgpu_logmel_device, alacgpu_fbank_device or
        alacgpu_mfcc_device call turns every row, the zeros behind its length included, into features.  Returns (feats float32 [B, 1 if mono else C,
        n_mels, features.frames(num_frames)], feat_lengths [B] int64 on the device: features.lengths(lengths) -- lengths // hop
        + 1 for a LogMel, fbank.fbank_lengths for a KaldiFbank --, -1 where lengths is -1); `out` is then the features tensor.
        ValueError: a spec.sample_rate that is not the rate of the crops, a dtype other than float32, num_frames below
        features.min_frames (n_fft // 2 + 1 for a LogMel; what gives no frame for a KaldiFbank).

        deltas: a deltas.Deltas -- Kaldi's add-deltas behind the features: the features go into a second scratch the corpus
        keeps and ONE alacgpu_deltas_device call writes feats [B, 1 if mono else C, (order + 1) * n_mels, frames] (`out` is
        then that tensor); feat_lengths are unchanged.  Bit for bit deltas.add_deltas(what the call returns without it, deltas,
        feat_lengths): a crop outside the corpus keeps its features as computed and gets zero deltas.  The stages behind it
        see (order + 1) * n_mels lines.  ValueError: no features=.

        vad: a vad.EnergyVad -- the last three steps of the Kaldi speaker recipes behind raw MFCCs, in Kaldi's order: ONE
        alacgpu_vad_energy_device call decides on feature line vad.line of the first channel of the features as they are
        behind the deltas and IN FRONT of normalize (compute-vad-decision on the raw features), into a scratch the corpus
        keeps; normalize runs over all frames (apply-cmvn-sliding); then ONE alacgpu_select_frames_device call moves the
        voiced frames of every line to its front, zeros behind them (select-voiced-frames).  feat_lengths are then the voiced
        counts, -1 stays -1, and augment sees those; nothing is read back.  Bit for bit vad.vad_energy, normalize.normalize and
        vad.select_frames applied in that order to what the call returns without vad= and normalize=.  The decisions are not
        returned.  ValueError: no features=, vad.line not below the line count in front of it.

        normalize: a normalize.MeanVar -- every line over its valid elements: lengths for PCM, feat_lengths for features, so a
        crop outside the corpus is zeros --, a normalize.TopDb -- every crop of features, or every channel of it with
        per_channel --, a sliding.SlidingMeanVar: Kaldi's sliding-window CMVN of every line, or a pcen.Pcen: per-channel energy
        normalisation of every line of mel or constant-Q energies over its feat_lengths frames, in place of the logarithm (one
        launch between the feature kernel and the selection and augment).  Bit for bit
        normalize.normalize(what the call returns without it, normalize, lengths).  ValueError: a TopDb without features, a
        MeanVar or a SlidingMeanVar with int32 crops, a SlidingMeanVar of a window above 7648 on lines of more than 16384
        elements; a Pcen without features=, with features that are not energies (a LogMel or a ConstantQ whose log is not
        None, a KaldiFbank with log=True, any KaldiMfcc), with deltas=, or with per-bin sequences of another length than the
        features have lines.

        augment: SpecAugment on the features, the last stage: an augment.SpecAugment, whose draws are then made here from the
        device's default generator (behind an AddNoise's and a Reverb's; with vad= for the voiced counts), or the pair (SpecAugment, draws) with the three
        tensors that its `draw(n_mels, feat_lengths)` returned.  Bit for bit augment.spec_augment(what the call returns without
        it, augment, feat_lengths); a crop outside the corpus (feat_lengths -1) is left as it is.  ValueError: no features=,
        draws that are not three int32 tensors [B, 2], [B, masks, 2], [B, masks, 2] on the corpus's device, a time warp of
        more than 16384 feature frames."""
        import torch

        plan = _stage_plan(self.channels, self.sample_rate, self._dev, dtype, num_frames, sample_rate, mono, speed=speed, pitch=pitch,
                           mix=mix, reverb=reverb, level=level, effects=effects, f0=f0, features=features, deltas=deltas, vad=vad,
                           normalize=normalize, augment=augment)
        B = None
        if plan.L is not None:
            self._open()
            B = int(files.shape[0]) if isinstance(files, torch.Tensor) and files.dim() == 1 else len(np.asarray(files))
            plan = _for_batch(plan, B, self._dev)
        return self._run(plan, files, frame_offsets, num_frames, B, dtype, out, check)

    def _run(self, plan, files, frame_offsets, num_frames, B, dtype, out, check):
        """`crops` behind its checks: `plan` is what `_stage_plan` returned, and `_for_batch` has seen it for the B crops (B None:
        a plan without a stage in front of the waveform, which has no L either).  Nothing of it is checked again."""
        import torch

        rate, Co, L, features, deltas, vad, f0 = plan.rate, plan.Co, plan.L, plan.features, plan.deltas, plan.vad, plan.f0
        # 1. the outputs: with features= `out` is theirs, and the waveform goes into the scratch they are computed from
        if features is not None:
            feats = self._out(out, (B, Co, plan.lines, plan.frames), torch.float32, zero=False)
            if deltas is not None:      # the features into a scratch, their deltas into what the call returns
                stacked, feats = feats, self._scratch("_delta_scratch", (B, Co, features.n_mels, plan.frames))
            out = self._scratch("_ft_scratch", (B, Co, L))
        # 2. the draws nobody gave, from the device's default generator; the companion crops, by the second corpora's own
        #    `crops`: the noise, then the responses
        if B is not None:
            plan = _middle_draws(plan, B, self._dev)
        pitch, mix, reverb, effects = plan.pitch, plan.mix, plan.reverb, plan.effects
        if mix is not None:
            nf, no, snr = mix[1]
            d_noise, noise_lengths = self._companion_crops(mix[0].noise, "_mix_scratch", nf, no, L, B=B, Co=Co, rate=rate,
                                                           check=check)
        if reverb is not None:
            draws = reverb[1]
            keep = draws[-1]
            if reverb[0].rooms is not None:       # simulated rooms: one channel, computed into the same scratch
                rooms = reverb[0].rooms
                if draws[0].shape[0] != B:
                    raise ValueError(f"the draws of reverb= are for {draws[0].shape[0]} crops, not {B}")
                d_rir = self._scratch("_reverb_scratch", (B, 1, reverb[0].frames(rate)))
                _, rir_lengths = _simulate(lambda: self._gpu, draws[0], draws[1], int(rate), reverb[0].frames(rate), rooms.taps,
                                           rooms.max_order, rooms.sound_speed, d_rir)
            else:
                from_0 = torch.zeros(B, dtype=torch.int64, device=self._dev)
                d_rir, rir_lengths = self._companion_crops(reverb[0].rirs, "_reverb_scratch", draws[0], from_0, reverb[0].frames(rate),
                                                           B=B, Co=Co, rate=rate, check=check)
        # 3. the waveform, once: into `out`, or into the scratch the features are computed from
        res, lengths = self._waveform(files, frame_offsets, num_frames, dtype=dtype, out=out, check=check, sample_rate=plan.sample_rate,
                                      mono=plan.mono, speed=plan.speed)
        # 4. the stages, in place and in this order on the same stream, by the corpus's own context
        ctx = lambda: self._gpu
        if pitch is not None and B:
            self._pitch(ctx, res, pitch, rate, lengths)
        if reverb is not None:
            _reverb(ctx, res, d_rir, lengths, torch.where(keep, rir_lengths, 0), res)
        if mix is not None:
            _mix(ctx, res, d_noise, lambda: snr_ratio(snr, B, self._dev), lengths, noise_lengths, res)
        if plan.level is not None:
            _level(ctx, res, plan.level, rate, lengths, res)
        if effects is not None:
            _biquad(ctx, res, effects[1][0], lengths, effects[1][1], effects[0].clamp, res)
        if f0 is not None:
            if isinstance(f0, KaldiPitch):
                track = _kaldi_pitch(ctx, res, f0, lengths, self._scratch("_f0_scratch", (B, Co, f0.lines, int(f0.frames(L)))))
            elif isinstance(f0, PYin):
                track = _pyin(ctx, res, f0, lengths, self._scratch("_f0_scratch", (B, Co, 3, int(f0.frames(L)))))
            else:
                track = _yin(ctx, res, f0, lengths, self._scratch("_f0_scratch", (B, Co, 2, int(f0.frames(L)))))
        if features is not None:
            if B:
                features.launch(self._gpu, res, B, Co, L, L, feats, torch.cuda.current_stream(self._dev).cuda_stream)
            res, lengths = feats, features.lengths(lengths)
        if deltas is not None:
            res = _add_deltas(ctx, res, deltas, lengths, stacked)
        if vad is not None:         # Kaldi's order: the decision on the raw features, the selection behind the CMVN
            voiced = self._scratch("_vad_scratch", ((res.shape[0] * res.shape[-1] + 3) // 4,)).view(torch.uint8)
            voiced = _vad_energy(ctx, res, vad, lengths, out=voiced[:res.shape[0] * res.shape[-1]].view(res.shape[0], res.shape[-1]))
        if plan.normalize is not None:
            _normalize(ctx, res, plan.normalize, lengths, res)
        if vad is not None:
            res, lengths = _select_frames(ctx, res, voiced, lengths, res)
        if plan.augment is not None:
            _spec_augment(ctx, res, plan.augment[0] if plan.augment[1] is None else plan.augment, lengths, res)
        return (res, lengths) if f0 is None else (res, lengths, track)

    def _waveform(self, files, frame_offsets, num_frames, dtype, out, check, sample_rate, mono, speed=None):
        """The crops themselves, what `crops` returns without a stage: through `_resampled_crops` with speed=, at another
        rate, as one channel of two, or of a corpus whose rates differ; else planned and decoded here"""
        import torch

        if self.sample_rate is None and sample_rate is None:
            raise ValueError(_NEEDS_RATE)
        if (speed is not None or self.sample_rate is None or (mono and self.channels == 2)
                or (sample_rate is not None and sample_rate != self.sample_rate)):
            return self._resampled_crops(files, frame_offsets, num_frames, dtype=dtype, out=out, check=check, sample_rate=sample_rate,
                                         mono=mono, speed=speed)
        dtype = _torch_dtype(torch, torch.float32 if dtype is None else dtype)
        L = _frame_count("num_frames", num_frames)
        if L >= 1 << 32:
            raise ValueError(f"num_frames {L} does not fit 32 bits")
        self._open()
        d_files, d_offs, from_host = self._indices(files, frame_offsets)
        B = int(d_files.shape[0])
        out = self._out(out, (B, self.channels, L), dtype, zero=True)
        self._last = 0
        if B == 0 or L == 0:
            lengths = torch.zeros(B, dtype=torch.int64, device=self._dev)
            if B and L == 0 and not from_host:     # (the kernel's length codes, without the kernel)
                lengths = torch.where(self._inside(d_files, d_offs, self._d_num_frames)[0], lengths, lengths - 1)
                if check:
                    self._raise_bad_length(lengths, d_files, d_offs)
            return out, lengths
        win = self._window(None, L)
        K = win["K"]
        if B * K >= 1 << 32:
            raise ValueError(f"{B} crops of up to {K} packets: a call plans fewer than 2^32 entries")
        lengths = self._plan_and_decode(d_files, d_offs, L, K, win["S"], out)
        if check:
            self._check_last(lengths, d_files, d_offs, L, K)
        return out, lengths

    def _pitch(self, ctx, res, pitch, rate, lengths):
        """crops(pitch=(spec, draws)) on the crops `res`, in place: the ratios of the draws, gathered on the device"""
        import torch

        spec, draws = pitch
        key = (spec.ratios, rate)
        if getattr(self, "_pitch_tables", None) is None or self._pitch_tables[0] != key:
            pq = np.array([[f.numerator, f.denominator] for f in spec.ratios], dtype=np.int32)
            self._pitch_tables = (key, _ratio_kinds(spec.ratios, int(rate)), torch.from_numpy(np.ascontiguousarray(pq[:, 0])).to(self._dev),
                                  torch.from_numpy(np.ascontiguousarray(pq[:, 1])).to(self._dev))
        _, kinds, d_ps, d_qs = self._pitch_tables
        k = draws.long().clamp(0, len(spec.ratios) - 1)
        names = dict(stretched="_pitch_scratch", resampled="_pitch_back_scratch")
        _pitch_shift(ctx, res, d_ps[k], d_qs[k], kinds, k.to(torch.int32), lengths, spec.n_fft, res,
                     lambda name, shape: self._scratch(names[name], shape))

    def _companion_crops(self, other, scratch, files, offsets, frames, B, Co, rate, check):
        """What a stage needs of a second corpus for B crops of Co channels at `rate`: other.crops(files, offsets, frames) at
        that rate, as one channel when other's channel count is not Co, into the scratch THIS corpus keeps under the
        attribute `scratch` -- so `other` may be this corpus.  Returns (the crops [B, Co or 1, frames], their lengths)."""
        if files.shape[0] != B:
            raise ValueError(f"{files.shape[0]} draws for {B} crops")
        view = self._scratch(scratch, (B, Co if other.channels == Co else 1, frames))
        return view, other.crops(files, offsets, frames, out=view, check=check, sample_rate=rate, mono=other.channels != Co)[1]

    def _out(self, out, shape, dtype, zero):
        """The tensor a call writes: `out` checked against shape and dtype, or a new one; zeroed where the decode relies on it"""
        import torch

        if out is None:
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self._dev)
        if (not isinstance(out, torch.Tensor) or out.shape != shape or out.dtype != dtype or out.device != self._dev
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on {self._dev}")
        return out.zero_() if zero else out

    def _scratch(self, name, shape):
        """A float32 view of `shape` on the flat scratch the corpus keeps under the attribute `name`, which grows when a call
        needs more"""
        import torch

        n = int(np.prod(shape))
        if getattr(self, name) is None or getattr(self, name).numel() < n:
            setattr(self, name, None)       # (the old one goes first)
            setattr(self, name, torch.empty(n, dtype=torch.float32, device=self._dev))
        return getattr(self, name)[:n].view(shape)

    @staticmethod
    def _at(files, draws, nk):
        """Where (file, drawn factor) is in a flat table [F * nk] of `_rate`: the file itself without draws"""
        return files if draws is None else files * nk + draws.long().clamp(0, nk - 1)

    def _inside(self, d_files, d_offs, d_totals, draws=None, nk=1):
        """Which crops are inside the corpus, on the device: (ok [B] bool -- a file index in 0 .. F - 1 and an offset in 0 ..
        its total --, `at`: where the crop's total is in d_totals, int64, from the file index clamped into 0 .. F - 1, and
        the totals gathered with it).  draws (int tensor [B]): d_totals is [F * nk], a file's total at each of nk factors;
        a crop's draw has to be in 0 .. nk - 1 as well, and `at` is file * nk + the draw, clamped."""
        f64 = d_files.long()
        ok = (f64 >= 0) & (f64 < self.num_files)
        if draws is not None:
            ok &= (draws >= 0) & (draws < nk)
        at = self._at(f64.clamp(0, self.num_files - 1), draws, nk)
        totals = d_totals[at]
        ok &= (d_offs >= 0) & (d_offs <= totals)
        return ok, at, totals

    def _plan_and_decode(self, d_files, d_offs, L, K, S, out, d_frames=None):
        """The launches of a step: the plan of the crops (d_files, d_offs) of L frames with K entries each, the staging of its
        packets (a tiered corpus: S bytes per crop) and the decode into out [B, C, L]; returns the planner's lengths.
        d_frames: a window length per crop (int32 device tensor, at most L each; alacgpu_plan_crops_frames_device)."""
        import torch

        B, C_ = int(d_files.shape[0]), self.channels
        n = B * K
        pl = self._plan_arrays(n)
        lengths = torch.empty(B, dtype=torch.int64, device=self._dev)
        stream = torch.cuda.current_stream(self._dev).cuda_stream
        ctx = self._gpu
        tables = (ctx._ctx, _dp(self._pkt_offset), _dp(self._pkt_size), _dp(self._pkt_end), _dp(self._file_first), _dp(self._file_cfg),
                  self.num_files, _dp(d_files), _dp(d_offs))
        plan = (B, L, K, C_ * L, _dp(pl["offsets"]), _dp(pl["sizes"]), _dp(pl["cfg_idx"]), _dp(pl["dst_first"]), _dp(pl["dst_frames"]),
                _dp(pl["src_skip"]), _dp(lengths), _VP(stream))
        if d_frames is None:
            _check(lib().alacgpu_plan_crops_device(*tables, *plan), ctx._ctx)
        else:
            _check(lib().alacgpu_plan_crops_frames_device(*tables, _dp(d_frames), *plan), ctx._ctx)
        blob, blob_bytes, offsets = self._blob, self._blob_bytes, pl["offsets"]
        if self._hi_bytes:
            # the packets of this step from both tiers into the staging blob, each at a multiple of 16; the decode reads that
            blob_bytes = B * S
            blob, sp = self._stage_arrays(n, blob_bytes)
            self._stage_bytes = blob_bytes
            offsets = sp["offsets"]
            ctx.stage_packets_device(self._blob if self._lo_bytes else None, self._lo_bytes, self._pinned.array.ctypes.data,
                                     self._hi_bytes, pl["offsets"], pl["sizes"], n, blob, blob_bytes, offsets, sp["total"],
                                     stream=stream)
        ctx.decode_window_into_device(blob, blob_bytes, offsets, pl["sizes"], pl["cfg_idx"], n, pl["dst_first"],
                                      pl["dst_frames"], pl["src_skip"], out, C_, "planar", L, None, pl["status"], stream=stream)
        self._last = n
        return lengths

    def resampled_frames(self, sample_rate, speed=None):
        """Ty_f: the frames of every file at sample_rate, ceil(b * T_f / a) with the file's own reduced ratio a : b (int64 host
        array [F]).  speed (a SpeedPerturb): int64 [F, len(speed.factors)], the file played at every factor."""
        if speed is not None and not isinstance(speed, SpeedPerturb):
            raise ValueError(f"speed must be a speed.SpeedPerturb, not {speed!r}")
        Ty = self._rate(sample_rate, speed)["Ty"]
        return Ty if speed is not None else Ty[:, 0]

    def _rate(self, sample_rate, speed=None):
        """What crops at sample_rate (None: the corpus's own rate) need, played at the factors of `speed` (a SpeedPerturb; None:
        the one factor 1), once per (rate, factors).  Every entry: rate; nk, the number of factors; Ty, int64 [F, nk] on the
        host, file f's frames at the rate at factor k, Ty_max [F], the most over the factors, and d_Ty, Ty flat on the device;
        a, b, width; and the filter tables d_d0, d_w.  The two variants of `_resampled_crops`:
          uniform   a corpus of one rate without speed: a, b, width are ints and d_d0, d_w the one table (resample.device_table).
          per crop  everything else.  A crop's kind is (its file's rate, its factor): the distinct rates (without speed in the
                    order they first appear, with it ascending: the order `desc` and `ratios` have had in either case),
                    rate_of [F] a file's, kind = rate_of * nk + factor.  Per kind, int64 host arrays [kinds]: a, b,
                    width -- without speed the table's (resample.rows_tables of the rates: desc on the host, d_desc, d_d0,
                    d_w), with it speed.ratio's --, and `ratios`, the same as the kernel's uint32 [kinds, 3] with a = 0, a
                    ratio that is skipped, at factor 1, whose crops go through the tables (d_ratios).  On the device d_kind
                    [F * nk], the kind of (file, factor), and d_kinds [kinds, 5], a kind's whole row for one gather: a, b,
                    width, its table (factor 1; else len(desc): a row of zeros) and its ratio (the kind itself; at factor 1
                    len(ratios): skipped).
        ValueError: a rate or a ratio the filters do not take, naming the first file whose table is too large (with speed, the
        place of its rate among the ascending rates)."""
        import torch

        from .resample import device_table, resampled_frames, rows_tables

        R = self.sample_rate if sample_rate is None else sample_rate
        if R is None and speed is not None:
            raise ValueError(_NEEDS_RATE)
        key = (R, None if speed is None else speed.factors)
        if key not in self._rates:
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self._dev)
            nk = 1 if speed is None else len(speed.factors)
            if self.sample_rate is not None and speed is None:
                rt = dict(zip(("a", "b", "width", "d_d0", "d_w"), device_table(self.sample_rate, R, self._dev)))
                Ty = resampled_frames(self.num_frames, rt["a"], rt["b"])[:, None]
            else:
                rates, first, rate_of = np.unique(self.sample_rates, return_index=True, return_inverse=True)
                rate_of = rate_of.reshape(-1)
                if speed is not None:
                    abw = np.array([_speed_ratio(int(r), f, R) for r in rates for f in speed.factors], dtype=np.int64)
                    if int(abw[:, 2].max()) > _SPEED_MAX_WIDTH:
                        raise ValueError(f"{int(rates.max())} Hz to {R} Hz: a filter of width {int(abw[:, 2].max())}, the kernel takes {_SPEED_MAX_WIDTH}")
                else:       # the rates, and so the tables, in the order they first appear among the files
                    order = np.argsort(first)
                    rates, first, rate_of = rates[order], first[order], np.argsort(order)[rate_of]
                try:
                    table_of, desc, d0, w = rows_tables(rates.tolist(), R)
                except ValueError as e:     # "source i: ...", i the rate's place: without speed the message names the rate's first file
                    i, colon, what = str(e).partition(":")
                    raise ValueError(f"source {first[int(i[7:])]}:{what}" if speed is None and colon and i[:7] == "source " else str(e)) from None
                if speed is None:
                    abw = desc[table_of, :3].astype(np.int64)
                kind = np.arange(len(abw))
                plain = kind % nk == (0 if speed is None else speed.one)
                ratios = abw.astype(np.uint32)
                ratios[plain] = (0, 1, 0)
                kinds = np.column_stack([abw, np.where(plain, table_of[kind // nk], len(desc)), np.where(plain, len(abw), kind)])
                kind_of = rate_of[:, None] * nk + np.arange(nk)
                a, b, width = abw.T
                Ty = resampled_frames(self.num_frames[:, None], a[kind_of], b[kind_of])
                rt = dict(a=a, b=b, width=width, rate_of=rate_of, desc=desc, ratios=ratios, d_kind=up(kind_of.reshape(-1)),
                          d_kinds=up(kinds), d_desc=up(desc.view(np.int32)), d_d0=up(d0), d_w=up(w), d_ratios=up(ratios.view(np.int32)))
            self._rates[key] = dict(rt, rate=R, nk=nk, Ty=Ty, Ty_max=Ty.max(axis=1), d_Ty=up(Ty.reshape(-1)))
        return self._rates[key]

    def _resampled_crops(self, files, frame_offsets, num_frames, dtype, out, check, sample_rate, mono, speed=None):
        """crops(..., sample_rate=R, mono=, speed=(spec, draws)): crop b is frames frame_offsets[b] .. + num_frames of file
        files[b], played at the factor k = draws[b] with speed=, RESAMPLED AS A WHOLE to R Hz (resample.py states the filter,
        speed.py the one without tables) by the reduced ratio a : b of its kind, zero behind its end; lengths[b] =
        min(num_frames, Ty - offset) with Ty = ceil(b * T_f / a), -1 for a file index, a draw or an offset outside -- the host
        checks and the device-tensor rule are those of `crops`, with Ty for T_f (with speed= the host checks against the
        file's largest Ty over the factors; the exact check is the device's).  A step: the source frames a crop needs
        (`source_window`: Ls(num_frames) of them from (o // b) * a - width on, clamped at 0, by integer operations on the
        device) are planned, staged and decoded as crops of the source into a zeroed float32 scratch [B, C, Ls] the corpus
        keeps, then the resample call filters every crop out of it.  mono: two channels become their mean in front of the
        filter.  dtype: float32 (ValueError otherwise).  The step has the two variants of `_rate`:
          uniform   a, b, width are ints; alacgpu_plan_crops_device; alacgpu_resample_device.  sample_rate None or the
                    corpus's own never comes here without `mono`; with it there is no filter, the kernel only takes the mean
                    (resample.identity_table).
          per crop  a, b, width, table and ratio are the crop's kind's row of d_kinds, one gather;
                    alacgpu_plan_crops_frames_device with the crop's own window in a scratch [B, C, the largest] (a crop of a
                    16 kHz file does not decode what a crop of a 48 kHz file needs); alacgpu_resample_rows_device with a
                    table per row for the crops at factor 1 -- so those are bit for bit what they are without speed=; a file
                    already at R goes through the table that copies --, every other row as zeros: a crop outside the corpus,
                    and the crops at another factor, which alacgpu_resample_ratio_rows_device then fills where there is
                    more than one factor; it skips the rest."""
        import torch

        if not _is_f32(torch, dtype):
            raise ValueError("crops at another sample rate or as mono are float32")
        L = _frame_count("num_frames", num_frames)
        self._open()
        if self.channels not in (1, 2):
            raise ValueError(_TWO_CHANNELS.format(n=self.channels))
        spec, draws = (None, None) if speed is None else speed
        rt = self._rate(sample_rate, spec)
        win = self._window(rt["rate"], L, spec)
        Ls, K = win["Ls_max"], win["K"]
        d_files, d_offs, _ = self._indices(files, frame_offsets, rt["Ty_max"])
        B, C_ = int(d_files.shape[0]), self.channels
        if spec is not None and draws is None:
            draws = spec.draw(B, device=self._dev)      # (given draws are B: `_cropstages._for_batch`)
        out = self._out(out, (B, 1 if mono else C_, L), torch.float32, zero=False)
        if B * K >= 1 << 32:
            raise ValueError(f"{B} crops of up to {K} packets: a call plans fewer than 2^32 entries")
        # the crops in source frames: where the target offset is inside its file, else an offset the planner refuses (-1)
        ok, at, Ty = self._inside(d_files, d_offs, rt["d_Ty"], draws, rt["nk"])
        rows = "d_kinds" in rt
        if rows:
            kind = rt["d_kind"][at]
            a, b, width, table, ratio = rt["d_kinds"][kind].unbind(1)
        else:
            a, b, width = rt["a"], rt["b"], rt["width"]
        origin = (torch.div(d_offs, b, rounding_mode="floor") * a - width).clamp(min=0)
        src_offs = torch.where(ok, origin, -1)
        lengths = torch.where(ok, (Ty - d_offs).clamp(max=L), -1)
        if B == 0 or L == 0:
            self._last = 0
            if check and B:
                self._raise_bad_length(lengths, d_files, d_offs)
            return out, lengths
        scratch = self._scratch("_rs_scratch", (B, C_, Ls))
        scratch.zero_()
        valid = self._plan_and_decode(d_files, src_offs, Ls, K, win["S"], scratch, d_frames=win["d_Ls"][kind] if rows else None)
        rows_of = (scratch, B, C_, Ls, origin, valid, d_offs, L)
        stream = torch.cuda.current_stream(self._dev).cuda_stream
        if not rows:
            self._gpu.resample_device(*rows_of, a, b, width, rt["d_d0"], rt["d_w"], mono, out, stream=stream)
        else:
            row_table = torch.where(ok, table, len(rt["desc"])).to(torch.int32)
            self._gpu.resample_rows_device(*rows_of, rt["desc"], rt["d_desc"], rt["d_d0"], rt["d_w"], row_table, mono, out, stream=stream)
            if rt["nk"] > 1:
                row_ratio = torch.where(ok, ratio, len(rt["ratios"])).to(torch.int32)
                self._gpu.resample_ratio_rows_device(*rows_of, rt["ratios"], rt["d_ratios"], row_ratio, mono, out, stream=stream)
        if check:
            self._check_last(valid, d_files, src_offs, Ls, K, d_shown=d_offs)
        return out, lengths

    def random_crops(self, batch, num_frames, generator=None, dtype=None, out=None, check=True, features=None, normalize=None,
                     mix=None, reverb=None, speed=None, pitch=None, f0=None, effects=None, level=None, deltas=None, vad=None, augment=None,
                     sample_rate=None, mono=False):
        """`batch` crops of num_frames frames drawn on the device: files uniform over the corpus, the first frame uniform in
        0 .. max(T_f - num_frames, 0).  generator: a torch.Generator (of the corpus's device, or of the CPU: then the draws are
        made there and uploaded).  Returns (pcm, lengths, files, frame_offsets), the draws as device int64 tensors.
        sample_rate / mono as for `crops`: the frames, T_f included, then count at sample_rate.  features as for `crops`:
        (feats, feat_lengths, files, frame_offsets).  deltas, vad and normalize as for `crops`: with vad= feat_lengths are the
        voiced counts, and nothing is read back for them.  mix as for `crops`; an AddNoise is drawn from
        `generator`, behind the call's own two draws (AddNoise.draw states its four).  reverb as for `crops`; a Reverb is
        drawn from `generator` behind those (Reverb.draw states its two).  effects as for `crops`; an Effects is drawn from
        `generator` behind those (Effects.draw states its draws).  level as for `crops`: it draws nothing.  augment as for `crops`; a SpecAugment is drawn from
        `generator` behind those, for the feat_lengths the call returns (augment.py states its draws) -- with vad= for the
        lengths in front of the selection, which are known without the device's decisions.  speed as for `crops`;
        a SpeedPerturb is drawn from `generator` behind the call's own two draws and in front of an AddNoise's
        (SpeedPerturb.draw states its two), and the first frame is then uniform in 0 .. max(Ty[f, k] - num_frames, 0), from the
        same u, with the frames of the file at its factor.  pitch as for `crops`; a PitchShift is drawn from `generator` behind a
        SpeedPerturb's and in front of an AddNoise's (PitchShift.draw states its two).  f0 as for `crops`: it draws nothing, and the
        result gains the track at its end: (pcm or feats, lengths, files, frame_offsets, track)."""
        import torch

        B, L = _frame_count("batch", batch), _frame_count("num_frames", num_frames)
        plan = _stage_plan(self.channels, self.sample_rate, self._dev, dtype, num_frames, sample_rate, mono, speed=speed, pitch=pitch,
                           mix=mix, reverb=reverb, level=level, effects=effects, f0=f0, features=features, deltas=deltas, vad=vad,
                           normalize=normalize, augment=augment)
        if self.sample_rate is None and sample_rate is None:
            raise ValueError(_NEEDS_RATE)
        if plan.L is not None:
            self._open()
            plan = _for_batch(plan, B, self._dev)
        dev = generator.device if generator is not None else self._dev
        files = torch.randint(0, self.num_files, (B,), generator=generator, device=dev, dtype=torch.int64).to(self._dev)
        u = torch.rand(B, generator=generator, device=dev, dtype=torch.float64).to(self._dev)
        spec, draws = (None, None) if plan.speed is None else plan.speed
        if spec is not None and draws is None:
            draws = spec.draw(B, generator=generator, device=self._dev)
            plan = plan._replace(speed=(spec, draws))
        if sample_rate is None and spec is None:    # the native crops: the files' own frames, and nothing to upload
            ends = self._d_num_frames[files]
        else:                                       # the frames of the crop's file at the rate of the crops, played at its factor
            rt = self._rate(sample_rate, spec)
            ends = rt["d_Ty"][self._at(files, draws, rt["nk"])]
        span = (ends - L).clamp(min=0)
        offs = torch.minimum(torch.floor(u * (span + 1).to(torch.float64)).to(torch.int64), span)
        plan = _middle_draws(plan, B, self._dev, generator)
        augment = plan.augment
        if augment is not None and augment[1] is None:      # for the feat_lengths the call is going to return
            feat_lengths = plan.features.lengths((ends - offs).clamp(max=L))
            plan = plan._replace(augment=(augment[0], augment[0].draw(plan.lines, feat_lengths, generator=generator)))
        res = self._run(plan, files, offs, L, B, dtype, out, check)
        return (res[0], res[1], files, offs) + tuple(res[2:])

    def last_staged_bytes(self):
        """The bytes the last crops call of a tiered corpus staged (every packet rounded up to 16): a device int64 tensor of one
        element, no synchronisation; None for a corpus without a host tier or before the first such call.  It is a view of an
        array the next call overwrites."""
        return self._stage_plan["total"] if self._stage_plan is not None else None

    def last_status(self):
        """The last crops call's per-entry statuses (ALACGPU_ST_*, as the kernels wrote them) and the mask of the entries that
        are packets (the others are padding): two device tensors of B * K entries, crop b's at b * K ..; no synchronisation.
        They are views of arrays the next call overwrites."""
        import torch

        if not self._last:
            return (torch.zeros(0, dtype=torch.int32, device=self._dev), torch.zeros(0, dtype=torch.bool, device=self._dev))
        return self._plan["status"][:self._last], self._plan["cfg_idx"][:self._last] != -1

    # -- check=True: one reduction on the device, one small read ------------------------------------------------------------------
    def _raise_bad_length(self, lengths, d_files, d_offs):
        import torch

        B = lengths.shape[0]
        first = int(torch.where(lengths < 0, torch.arange(B, device=self._dev), B).min())
        if first < B:
            self._bad_length(first, int(lengths[first]), d_files, d_offs)

    def _bad_length(self, b, code, d_files, d_offs):
        f, o = int(d_files[b]), int(d_offs[b])
        if code == -2:
            raise AlacGpuError(f"crop {b} (source {f}): more packets than the plan reserves per crop")
        raise ValueError(f"crop {b}: file {f} or frame offset {o} outside the corpus")

    def _check_last(self, lengths, d_files, d_offs, L, K, d_shown=None):
        """d_shown: the offsets a message about a crop outside the corpus names (default d_offs)"""
        import torch

        n, B, pl = self._last, lengths.shape[0], self._plan
        st, valid = pl["status"][:n], pl["cfg_idx"][:n] != -1
        # statuses as AlacContext.ReadBatch reads them (_normalise_status): the element type is the packet's first three bits
        if self._hi_bytes:      # (where the packet is now: in the staging blob)
            first_byte = self._stage[self._stage_plan["offsets"][:n].clamp(max=max(self._stage_bytes - 1, 0))]
        else:
            first_byte = self._blob[pl["offsets"][:n].clamp(max=max(self._blob_bytes - 1, 0))]
        mono = (first_byte >> 5) == 0
        ok = (st == ST_OK) | (st == ST_UNSUPPORTED_ELEMENT) | ((st == ST_UNSUPPORTED_PREDTYPE) & mono)
        bad_entry = torch.where(valid & ~ok, pl["iota"][:n], n).min()
        bad_crop = torch.where(lengths < 0, pl["iota"][:B], B).min()
        bad_entry, bad_crop = (int(x) for x in torch.stack([bad_entry, bad_crop]).cpu())      # the one read
        if bad_crop < B:
            self._bad_length(bad_crop, int(lengths[bad_crop]), d_files, d_offs if d_shown is None else d_shown)
        if bad_entry < n:
            b, i = divmod(bad_entry, K)
            f, o = int(d_files[b]), int(d_offs[b])
            h = self._host
            g0, g1 = int(h["file_first"][f]), int(h["file_first"][f + 1])
            ends = h["pkt_end"][g0:g1].astype(np.int64)
            p0 = 0 if o == 0 else int(np.searchsorted(ends, o, side="right"))
            raise AlacGpuError(f"crop {b} (source {f}), packet {p0 + i} does not decode: {_status_text(int(st[bad_entry]))}")
