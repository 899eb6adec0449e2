"""alac.net_amd -- MI355X-native ALAC frame-decode path (teekay/ALAC.NET's AlacFile.DecodeFrame).

Python host side over the C ABI of include/alacgpu.h (libalacgpu.so: hand-written gfx950 HIP
kernels).  It mirrors the reference's interface for the path -- `AlacFile(samplesize,
numchannels)`, `SetInfo(codecData)`, `DecodeFrame(inbuffer, outbuffer)` (AlacFile.cs:16,:63,:428)
-- and adds the batch entry points.  There is NO CPU fallback: if libalacgpu.so is missing or no
gfx950 GPU is usable, every entry point raises.
"""
import ctypes as C
import operator
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("ALACGPU_LIB", os.path.join(_HERE, "csrc", "libalacgpu.so"))  # override: A/B builds only
_LIB = None

# per-packet status codes (include/alacgpu.h)
ST_OK, ST_UNSUPPORTED_ELEMENT, ST_UNSUPPORTED_SAMPLE_SIZE, ST_UNSUPPORTED_PREDTYPE = 0, 1, 2, 3
ST_BAD_SAMPLE_COUNT, ST_OVERRUN, ST_REF_THROWS, ST_UNSUPPORTED_PARAMS = 4, 5, 6, 7
ST_DEST_RANGE = 8
# alacgpu_decode_into_device: destination layout and element type
DST_INTERLEAVED, DST_PLANAR = 0, 1
DST_INT32, DST_FLOAT32 = 0, 1
_LAYOUTS = {"interleaved": DST_INTERLEAVED, "planar": DST_PLANAR}
MAX_FRAME = 16384   # the longest frame the reference decodes (its scratch, AlacFile.cs:28)

CFG_DTYPE = np.dtype(
    [
        ("max_samples_per_frame", "<u4"),
        ("sample_size", "u1"),
        ("rice_history_mult", "u1"),
        ("rice_initial_history", "u1"),
        ("rice_kmodifier", "u1"),
        ("num_channels", "u1"),
        ("ctor_sample_size", "u1"),
        ("reserved", "u1"),
        ("_pad", "u1"),
    ]
)
assert CFG_DTYPE.itemsize == 12

# every symbol include/alacgpu.h declares: (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "alacgpu_version": (C.c_int, []),
    "alacgpu_device_count": (C.c_int, []),
    "alacgpu_alloc_pinned": (_VP, [C.c_size_t]),
    "alacgpu_free_pinned": (None, [_VP]),
    "alacgpu_create": (C.c_int, [_VP, C.c_uint32, C.c_int, C.POINTER(_VP)]),
    "alacgpu_destroy": (None, [_VP]),
    "alacgpu_cfg_from_codec_data": (C.c_int, [_VP, C.c_uint32, C.c_int, C.c_int, _VP]),
    "alacgpu_decode_batch": (C.c_int, [_VP, _VP, C.c_uint64, _VP, _VP, _VP, C.c_uint32, _VP, C.c_uint32, _VP, _VP, _VP]),
    "alacgpu_decode_batch_sharded": (C.c_int, [_VP, C.c_uint32, _VP, C.c_uint64, _VP, _VP, _VP, C.c_uint32, _VP, C.c_uint32, _VP,
                                               _VP, _VP]),
    "alacgpu_decode_batch_device": (C.c_int, [_VP, _VP, C.c_uint64, _VP, _VP, _VP, C.c_uint32, _VP, C.c_uint32, _VP,
                                              _VP, _VP, _VP]),
    "alacgpu_decode_into_device": (C.c_int, [_VP, _VP, C.c_uint64, _VP, _VP, _VP, C.c_uint32, _VP, _VP, _VP, C.c_uint64,
                                             C.c_uint32, C.c_int, C.c_int, C.c_uint64, _VP, _VP, _VP]),
    "alacgpu_decode_window_into_device": (C.c_int, [_VP, _VP, C.c_uint64, _VP, _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP,
                                                    C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint64, _VP, _VP, _VP]),
    "alacgpu_plan_crops_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alacgpu_plan_crops_frames_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP, _VP, C.c_uint32, C.c_uint32,
                                                   C.c_uint32, C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alacgpu_compact_packets_device": (C.c_int, [_VP, _VP, C.c_uint64, _VP, C.c_uint32, _VP, C.c_uint64, C.c_uint64, _VP, _VP, _VP]),
    "alacgpu_stage_packets_device": (C.c_int, [_VP, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP, C.c_uint32, _VP, C.c_uint64, _VP, _VP,
                                               _VP]),
    "alacgpu_resample_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, _VP, _VP, _VP, C.c_uint64, C.c_uint32, C.c_uint32,
                                          C.c_uint32, _VP, _VP, C.c_int, _VP, _VP]),
    "alacgpu_resample_rows_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, _VP, _VP, _VP, C.c_uint64, _VP, _VP,
                                               C.c_uint32, _VP, _VP, _VP, C.c_int, _VP, _VP]),
    "alacgpu_resample_ratio_rows_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, _VP, _VP, _VP, C.c_uint64, _VP, _VP,
                                                     C.c_uint32, _VP, C.c_int, _VP, _VP]),
    "alacgpu_logmel_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _VP,
                                        _VP, _VP, C.c_int, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_fbank_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       _VP, _VP, _VP, C.c_uint32, C.c_float, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_mfcc_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_float, C.c_float, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_deltas_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _VP,
                                        C.c_uint32, C.c_uint32, _VP, _VP]),
    "alacgpu_normalize_meanvar_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, C.c_int, C.c_int,
                                                   C.c_float, _VP]),
    "alacgpu_normalize_top_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_float, C.c_float,
                                               C.c_float, C.c_int, _VP]),
    "alacgpu_normalize_sliding_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, C.c_uint32,
                                                   C.c_uint32, C.c_int, C.c_int, _VP]),
    "alacgpu_pcen_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_float, C.c_float, C.c_float, _VP, C.c_uint32, C.c_int, _VP]),
    "alacgpu_vad_energy_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _VP, C.c_float, C.c_float,
                                            C.c_uint32, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_select_frames_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, _VP, C.c_uint64,
                                               _VP, _VP]),
    "alacgpu_mix_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _VP, _VP,
                                     _VP, _VP]),
    "alacgpu_biquad_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, _VP, C.c_uint32, _VP, C.c_int,
                                        _VP]),
    "alacgpu_level_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, C.c_uint32, C.c_uint32, _VP,
                                       C.c_double, C.c_double, C.c_int, _VP, _VP, _VP, _VP]),
    "alacgpu_yin_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_pyin_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _VP, _VP, _VP, _VP,
                                      _VP, _VP, C.c_uint64, C.c_int, _VP]),
    "alacgpu_kaldi_pitch_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP] + [C.c_uint32] * 17 +
                                   [_VP, _VP, _VP, _VP, C.c_uint64, C.c_int, _VP]),
    "alacgpu_cqt_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _VP, _VP, _VP,
                                     C.c_int, C.c_int, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_stft_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _VP, _VP, C.c_int,
                                      C.c_uint32, _VP, _VP, _VP, C.c_int, C.c_float, _VP, C.c_uint64, _VP]),
    "alacgpu_reverb_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                        C.c_uint64, _VP, _VP, _VP]),
    "alacgpu_rir_shoebox_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int32, C.c_double, _VP,
                                             C.c_uint64, _VP, _VP]),
    "alacgpu_time_stretch_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _VP,
                                              _VP, _VP, _VP, C.c_uint32, _VP]),
    "alacgpu_copy_rows_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _VP, _VP]),
    "alacgpu_specaugment_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _VP, _VP, _VP,
                                             C.c_uint32, _VP, C.c_uint32, C.c_float, _VP]),
    "alacgpu_encode_max_packet_bytes": (C.c_size_t, [C.c_uint32, C.c_int, C.c_int]),
    "alacgpu_encode_device": (C.c_int, [_VP, _VP, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint64, _VP, _VP, _VP, C.c_uint32,
                                        _VP, C.c_uint64, _VP, _VP, _VP]),
    "alacgpu_decode_frame": (C.c_int, [_VP, C.c_uint32, _VP, C.c_uint32, _VP, C.c_uint32, _VP, _VP]),
    "alacgpu_expand_reference_layout": (C.c_size_t, [_VP, _VP, C.c_int32, _VP]),
    "alacgpu_format_samples": (C.c_size_t, [C.c_int, _VP, C.c_int32, _VP]),
    "alacgpu_last_kernel_ms": (C.c_float, [_VP]),
    "alacgpu_set_output_format": (C.c_int, [_VP, C.c_int]),
    "alacgpu_set_pairing": (C.c_int, [_VP, C.c_int]),
    "alacgpu_pairing_stats": (C.c_int, [_VP, _VP]),
    "alacgpu_pairing_shift_starts": (C.c_int, [_VP]),
    "alacgpu_strerror": (C.c_char_p, [C.c_int]),
    "alacgpu_status_string": (C.c_char_p, [C.c_int]),
    "alacgpu_last_error": (C.c_char_p, [_VP]),
    "alacgpu_ctx_device": (C.c_int, [_VP]),
    "alacgpu_shard_ranges": (C.c_int, [_VP, C.c_uint32, C.c_uint32, _VP]),
    "alacgpu_comm_get_unique_id": (C.c_int, [_VP]),
    "alacgpu_comm_create": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.POINTER(_VP)]),
    "alacgpu_comm_destroy": (None, [_VP]),
    "alacgpu_comm_rank": (C.c_int, [_VP]),
    "alacgpu_comm_world": (C.c_int, [_VP]),
    "alacgpu_comm_last_error": (C.c_char_p, [_VP]),
    "alacgpu_allgather_pcm": (C.c_int, [_VP, _VP, _VP, C.c_uint32, _VP]),
    "alacgpu_decode_allgather_device": (C.c_int, [_VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP, _VP,
                                                  C.c_uint32, _VP]),
}


class AlacGpuError(RuntimeError):
    pass


class _Closing:
    """close() at the end of a with-block, and when the object is collected."""

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lib():
    """Load libalacgpu.so (built by __graft_entry__.build()).  Fails loudly: no fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIBPATH):
            raise AlacGpuError(
                f"{_LIBPATH} is missing: build it with `make -C alac.net_amd/csrc` "
                "(or __graft_entry__.build()).  There is no CPU fallback."
            )
        L = C.CDLL(_LIBPATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data_as(_VP) if a is not None else None


def _dp(t):
    """A torch device tensor's address (None stays NULL)."""
    return _VP(t.data_ptr()) if t is not None else None


def _pcm_view(name, t, layout):
    """The element type and layout codes of a PCM tensor argument (decode_into_device, encode_device); ValueError for a tensor
    the library cannot take."""
    import torch

    dtype = {torch.int32: DST_INT32, torch.float32: DST_FLOAT32}.get(t.dtype)
    if dtype is None:
        raise ValueError(f"{name} must be torch.int32 or torch.float32, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a device tensor")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be 'interleaved' or 'planar', not {layout!r}")
    return dtype, _LAYOUTS[layout]


def _status_text(st):
    return f"status {int(st)} ({lib().alacgpu_status_string(int(st)).decode()})"


def _raise_reference_exception(st, sample_size):
    """The exception the reference throws where DecodeFrame ends with status `st` (AlacFile.cs:574,:650,:660,:715); no
    exception for the others."""
    if st == ST_UNSUPPORTED_SAMPLE_SIZE:
        raise Exception("FIXME: unimplemented sample size " + str(sample_size))
    if st == ST_UNSUPPORTED_PREDTYPE:
        raise Exception("FIXME: unhandled predicition type")
    if st in (ST_BAD_SAMPLE_COUNT, ST_OVERRUN):
        raise IndexError("Index was outside the bounds of the array.")
    if st == ST_REF_THROWS:
        raise ValueError("Destination array was not long enough.")
    if st == ST_UNSUPPORTED_PARAMS:
        raise Exception("unsupported parameter combination")


def make_cfgs(rows):
    """rows: iterable of (max_samples_per_frame, sample_size, pb, mb, kb, num_channels) tuples or dicts."""
    if isinstance(rows, np.ndarray) and rows.dtype == CFG_DTYPE:
        return np.ascontiguousarray(rows)
    arr = np.zeros(len(rows), dtype=CFG_DTYPE)
    for i, r in enumerate(rows):
        if isinstance(r, dict):
            for k, v in r.items():
                arr[i][k] = v
        else:
            (arr[i]["max_samples_per_frame"], arr[i]["sample_size"], arr[i]["rice_history_mult"],
             arr[i]["rice_initial_history"], arr[i]["rice_kmodifier"], arr[i]["num_channels"]) = r
    return arr


def _check(rc, ctx=None):
    if rc != 0:
        L = lib()
        msg = L.alacgpu_strerror(rc).decode()
        if ctx:
            detail = L.alacgpu_last_error(ctx).decode()
            if detail:
                msg += f" ({detail})"
        raise AlacGpuError(f"alacgpu rc={rc}: {msg}")


def _check_comm(rc, comm):
    if rc != 0:
        L = lib()
        raise AlacGpuError(f"alacgpu rc={rc}: {L.alacgpu_strerror(rc).decode()} ({L.alacgpu_comm_last_error(comm).decode()})")


def _host_batch(cfgs, blob, offsets, sizes, cfg_idx, slot_ints, out):
    """The host-buffer decodes' arrays: returns the C call's arguments from `blob` on, and the outputs (pcm[n, slot_ints],
    out_bytes[n], out_samples[n], status[n]); `out` is the pcm array to decode into, if given."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    ci = None if cfg_idx is None else np.ascontiguousarray(cfg_idx, dtype=np.uint16)
    n = len(sizes)
    if slot_ints is None:
        slot_ints = int(max(int(c["max_samples_per_frame"]) * int(c["num_channels"]) for c in cfgs))
    pcm = out if out is not None else np.zeros((n, slot_ints), dtype=np.int32)
    if pcm.dtype != np.int32 or pcm.shape != (n, slot_ints) or not pcm.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous int32 array of shape (n_packets, slot_ints)")
    outs = (pcm, np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    args = (_ptr(blob), blob.size, _ptr(offsets), _ptr(sizes), _ptr(ci), n, _ptr(pcm), slot_ints) + tuple(_ptr(a) for a in outs[1:])
    return args, outs


class AlacGpuContext(_Closing):
    """Owns one alacgpu_ctx (one per host thread; calls are blocking unless stated)."""

    def __init__(self, cfgs, device=0):
        self._ctx = _VP()
        self.cfgs = make_cfgs(cfgs)
        L = lib()
        rc = L.alacgpu_create(_ptr(self.cfgs), len(self.cfgs), device, C.byref(self._ctx))
        if rc != 0:
            self._ctx = _VP()
        _check(rc)
        self.device = device

    def close(self):
        if self._ctx:
            lib().alacgpu_destroy(self._ctx)
            self._ctx = _VP()

    # -- host buffers: H2D + kernel + D2H ---------------------------------------------------------
    def decode_batch(self, blob, offsets, sizes, cfg_idx=None, slot_ints=None, out=None):
        """Returns (pcm[n, slot_ints] int32, out_bytes[n], out_samples[n], status[n]).  `out`: a pcm array to decode
        into instead of a fresh one (a fresh 100+ MB array costs more in page faults than the whole decode)."""
        args, outs = _host_batch(self.cfgs, blob, offsets, sizes, cfg_idx, slot_ints, out)
        _check(lib().alacgpu_decode_batch(self._ctx, *args), self._ctx)
        return outs

    # -- device buffers (torch tensors on this device), asynchronous on `stream` --------------------
    def decode_batch_device(self, d_blob, blob_bytes, d_offsets, d_sizes, d_cfg_idx, n_packets, d_pcm, slot_ints,
                            d_out_bytes, d_out_samples, d_status, stream=0):
        """All d_* are torch CUDA tensors (or None where the header allows NULL); `stream` is a raw
        hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream)."""
        rc = lib().alacgpu_decode_batch_device(self._ctx, _dp(d_blob), blob_bytes, _dp(d_offsets), _dp(d_sizes),
                                               _dp(d_cfg_idx), n_packets, _dp(d_pcm), slot_ints, _dp(d_out_bytes),
                                               _dp(d_out_samples), _dp(d_status), _VP(stream))
        _check(rc, self._ctx)

    def decode_into_device(self, d_blob, blob_bytes, d_offsets, d_sizes, d_cfg_idx, n_packets, d_dst_first, d_dst_frames, out,
                           channels, layout="planar", plane_stride=0, d_out_samples=None, d_status=None, stream=0):
        """alacgpu_decode_into_device: packet p's frames land at d_dst_first[p] of the gap-free tensor `out` (torch int32 or
        float32 on this device, contiguous; its dtype picks the element type), interleaved ((first + i) * channels + c) or
        planar (c * plane_stride + first + i).  d_* are torch device tensors (d_cfg_idx / d_out_samples may be None);
        asynchronous on `stream` (raw hipStream_t)."""
        dtype, lay = _pcm_view("out", out, layout)
        if d_status is None:
            raise ValueError("d_status is required")
        rc = lib().alacgpu_decode_into_device(self._ctx, _dp(d_blob), blob_bytes, _dp(d_offsets), _dp(d_sizes), _dp(d_cfg_idx),
                                              n_packets, _dp(d_dst_first), _dp(d_dst_frames), _dp(out), out.numel(), channels, lay,
                                              dtype, plane_stride, _dp(d_out_samples), _dp(d_status), _VP(stream))
        _check(rc, self._ctx)

    def decode_window_into_device(self, d_blob, blob_bytes, d_offsets, d_sizes, d_cfg_idx, n_packets, d_dst_first, d_dst_frames,
                                  d_src_skip, out, channels, layout="planar", plane_stride=0, d_out_samples=None, d_status=None,
                                  stream=0):
        """alacgpu_decode_window_into_device: decode_into_device with packet p's run starting d_src_skip[p] frames into the
        packet (an int32 device tensor, at most 16384 each; None: no skip, exactly decode_into_device): frames
        d_src_skip[p] .. + d_dst_frames[p] land at d_dst_first[p] of `out`."""
        dtype, lay = _pcm_view("out", out, layout)
        if d_status is None:
            raise ValueError("d_status is required")
        rc = lib().alacgpu_decode_window_into_device(self._ctx, _dp(d_blob), blob_bytes, _dp(d_offsets), _dp(d_sizes),
                                                     _dp(d_cfg_idx), n_packets, _dp(d_dst_first), _dp(d_dst_frames),
                                                     _dp(d_src_skip), _dp(out), out.numel(), channels, lay, dtype, plane_stride,
                                                     _dp(d_out_samples), _dp(d_status), _VP(stream))
        _check(rc, self._ctx)

    def encode_device(self, pcm, channels, d_src_first, d_src_frames, d_cfg_idx, n_packets, d_packets, slot_bytes, d_sizes,
                      d_status, layout="planar", plane_stride=0, stream=0):
        """alacgpu_encode_device: packet p encodes frames d_src_first[p] .. + d_src_frames[p] of `pcm` (torch int32 or float32
        on this device, contiguous; its dtype picks the element type) with stream cfg d_cfg_idx[p]; its bytes land at
        d_packets[p * slot_bytes:] (a uint8 device tensor), its size in d_sizes[p], its status in d_status[p].  d_* are torch
        device tensors; asynchronous on `stream` (raw hipStream_t).  Samples are taken as `save` takes them: int32 clamped to
        the cfg's sample range; float32 times 2^(bits-1) (in float32), clamped, then rounded half to even; NaN the smallest
        sample."""
        dtype, lay = _pcm_view("pcm", pcm, layout)
        rc = lib().alacgpu_encode_device(self._ctx, _dp(pcm), pcm.numel(), channels, lay, dtype, plane_stride, _dp(d_src_first),
                                         _dp(d_src_frames), _dp(d_cfg_idx), n_packets, _dp(d_packets), slot_bytes, _dp(d_sizes),
                                         _dp(d_status), _VP(stream))
        _check(rc, self._ctx)

    def compact_packets_device(self, d_packets, slot_bytes, d_sizes, n_packets, d_blob, base, blob_capacity, d_pkt_offset, d_total,
                               stream=0):
        """alacgpu_compact_packets_device: the packets the encoder left in slots (packet p at d_packets[p * slot_bytes:], its
        size in d_sizes[p]) back to back into d_blob from byte `base` on; d_pkt_offset[p] (int64 device tensor) = base + the
        sizes in front of p, d_total[0] (int64 device tensor) the sum of the sizes.  A packet that would end behind
        blob_capacity is not copied (offsets and total are complete all the same); nothing of d_blob outside the copied
        packets is written.  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_compact_packets_device(self._ctx, _dp(d_packets), slot_bytes, _dp(d_sizes), n_packets, _dp(d_blob), base,
                                                  blob_capacity, _dp(d_pkt_offset), _dp(d_total), _VP(stream))
        _check(rc, self._ctx)

    def stage_packets_device(self, d_blob_lo, lo_bytes, blob_hi, hi_bytes, d_src_offset, d_sizes, n_packets, d_stage, stage_capacity,
                             d_stage_offset, d_total, stream=0):
        """alacgpu_stage_packets_device: gather the n_packets packets at d_src_offset / d_sizes (int64 / int32 device tensors,
        a plan's) out of the source space -- d_blob_lo (a device tensor or None) first, blob_hi (a device tensor, the address
        of page-locked host memory, or None) behind it -- into d_stage (uint8 device tensor), each at the next multiple of
        16; d_stage_offset[j] (int64 device tensor) = where packet j went, d_total[0] the bytes all of them take.  A packet
        that would end behind stage_capacity is not copied.  Asynchronous on `stream` (raw hipStream_t); nothing is read
        back."""
        hi = _dp(blob_hi) if hasattr(blob_hi, "data_ptr") else (_VP(blob_hi) if blob_hi else None)
        rc = lib().alacgpu_stage_packets_device(self._ctx, _dp(d_blob_lo), lo_bytes, hi, hi_bytes, _dp(d_src_offset), _dp(d_sizes),
                                                n_packets, _dp(d_stage), stage_capacity, _dp(d_stage_offset), _dp(d_total), _VP(stream))
        _check(rc, self._ctx)

    def resample_device(self, d_src, rows, channels, src_stride, d_src_origin, d_src_valid, d_out_first, out_frames, a, b, width,
                        d_d0, d_weights, mono, d_out, stream=0):
        """alacgpu_resample_device: d_src (float32 device tensor, planar [rows, channels, src_stride]) resampled by a : b with
        the table d_d0 / d_weights (resample.device_table) into d_out (float32 [rows, 1 if mono else channels, out_frames],
        every element written).  Row r holds the source frames d_src_origin[r] .. + d_src_valid[r] of a signal that is zero
        elsewhere, and its output starts at target frame d_out_first[r] (three int64 device tensors).  Asynchronous on
        `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_resample_device(self._ctx, _dp(d_src), rows, channels, src_stride, _dp(d_src_origin), _dp(d_src_valid),
                                           _dp(d_out_first), out_frames, a, b, width, _dp(d_d0), _dp(d_weights), int(bool(mono)),
                                           _dp(d_out), _VP(stream))
        _check(rc, self._ctx)

    def resample_rows_device(self, d_src, rows, channels, src_stride, d_src_origin, d_src_valid, d_out_first, out_frames, tables,
                             d_tables, d_d0, d_weights, d_row_table, mono, d_out, stream=0):
        """alacgpu_resample_rows_device: resample_device with a table per row.  tables: the descriptors on the host, a uint32
        array [n_tables, 5] of (a, b, width, where the table's d0 starts in d_d0, where its weights start in d_weights:
        resample.device_tables); d_tables: the same on the device (int32 device tensor); d_row_table[r] (int32 device tensor,
        read as unsigned): the table of row r, n_tables and above for a row of zeros.  Asynchronous on `stream` (raw
        hipStream_t); nothing is read back."""
        tables = np.ascontiguousarray(tables, dtype=np.uint32).reshape(-1, 5)
        rc = lib().alacgpu_resample_rows_device(self._ctx, _dp(d_src), rows, channels, src_stride, _dp(d_src_origin),
                                                _dp(d_src_valid), _dp(d_out_first), out_frames, _ptr(tables), _dp(d_tables),
                                                len(tables), _dp(d_d0), _dp(d_weights), _dp(d_row_table), int(bool(mono)),
                                                _dp(d_out), _VP(stream))
        _check(rc, self._ctx)

    def resample_ratio_rows_device(self, d_src, rows, channels, src_stride, d_src_origin, d_src_valid, d_out_first, out_frames, ratios,
                                   d_ratios, d_row_ratio, mono, d_out, stream=0):
        """alacgpu_resample_ratio_rows_device: resample_device without tables, a ratio per row and every weight evaluated per
        tap (speed.py states the arithmetic).  ratios: the ratios on the host, a uint32 array [n_ratios, 3] of (a, b, width);
        d_ratios: the same on the device (int32 device tensor); d_row_ratio[r] (int32 device tensor, read as unsigned): the
        ratio of row r -- n_ratios and above, or a ratio with a == 0: the row is skipped, its part of d_out left as it is.
        Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        ratios = np.ascontiguousarray(ratios, dtype=np.uint32).reshape(-1, 3)
        rc = lib().alacgpu_resample_ratio_rows_device(self._ctx, _dp(d_src), rows, channels, src_stride, _dp(d_src_origin),
                                                      _dp(d_src_valid), _dp(d_out_first), out_frames, _ptr(ratios), _dp(d_ratios),
                                                      len(ratios), _dp(d_row_ratio), int(bool(mono)), _dp(d_out), _VP(stream))
        _check(rc, self._ctx)

    def logmel_device(self, d_src, rows, channels, src_stride, frames, n_fft, hop, n_mels, d_window, d_basis, d_fb, log_mode, floor,
                      d_out, out_frames, stream=0):
        """alacgpu_logmel_device: the log-mel features of d_src (float32 device tensor, planar [rows, channels, src_stride], the
        first `frames` of a plane are signal) into d_out (float32 [rows, channels, n_mels, out_frames], out_frames =
        1 + frames // hop, every element written) with the tables d_window [n_fft], d_basis [n_fft, 2 * (n_fft // 2 + 1)] and
        d_fb [n_mels, n_fft // 2 + 1] (features.LogMel builds them); log_mode 0: mel power, 1: ln, 2: log10 of
        max(., floor).  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_logmel_device(self._ctx, _dp(d_src), rows, channels, src_stride, frames, n_fft, hop, n_mels, _dp(d_window),
                                         _dp(d_basis), _dp(d_fb), log_mode, floor, _dp(d_out), out_frames, _VP(stream))
        _check(rc, self._ctx)

    def cqt_device(self, d_src, rows, channels, src_stride, frames, hop, n_bins, lengths, d_lengths, d_table, power, log_mode, floor,
                   d_out, out_frames, stream=0):
        """alacgpu_cqt_device: the constant-Q features of d_src (float32 device tensor, planar [rows, channels, src_stride], the
        first `frames` of a plane are signal) into d_out (float32 [rows, channels, n_bins, out_frames], out_frames =
        1 + frames // hop, every element written); lengths: the N_k [n_bins] (host), d_lengths the same on the device (int32),
        d_table the kernels in blocks of 16 bins (cqt.ConstantQ builds them); power 1: magnitude, 2: power; log_mode 0: none,
        1: ln, 2: log10 of max(., floor).  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if lengths.shape != (n_bins,):
            raise ValueError(f"lengths must be {n_bins} integers, not {lengths.shape}")
        rc = lib().alacgpu_cqt_device(self._ctx, _dp(d_src), rows, channels, src_stride, frames, hop, n_bins, _ptr(lengths), _dp(d_lengths),
                                      _dp(d_table), power, log_mode, floor, _dp(d_out), out_frames, _VP(stream))
        _check(rc, self._ctx)

    def stft_device(self, d_src, rows, channels, src_stride, frames, n_fft, hop, d_window, d_table, power, bands, d_bands, d_weights,
                    log_mode, floor, d_out, out_frames, stream=0):
        """alacgpu_stft_device: the spectrogram of d_src (float32 device tensor, planar [rows, channels, src_stride], the first
        `frames` of a plane are signal) into d_out (float32 [rows, channels, lines, out_frames], out_frames = 1 + frames // hop,
        every element written) with the tables d_window [n_fft] and d_table [n_fft, 2] (stft.Spectrogram builds them); power 0:
        the complex spectrum (lines 2 n_bins), 1: magnitude, 2: power (lines n_bins); bands: None, or the filterbank's (first,
        count, offset) per line [lines, 3] (host), d_bands the same on the device (int32) and d_weights the packed weights;
        log_mode 0: none, 1: ln, 2: log10 of max(., floor).  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        if bands is None:
            fb_lines, h_bands, d_bands, d_weights = 0, None, None, None
        else:
            bands = np.ascontiguousarray(bands, dtype=np.uint32)
            if bands.ndim != 2 or bands.shape[1] != 3:
                raise ValueError(f"bands must be [lines, 3], not {bands.shape}")
            fb_lines, h_bands, d_bands, d_weights = len(bands), _ptr(bands), _dp(d_bands), _dp(d_weights)
        rc = lib().alacgpu_stft_device(self._ctx, _dp(d_src), rows, channels, src_stride, frames, n_fft, hop, _dp(d_window), _dp(d_table),
                                       power, fb_lines, h_bands, d_bands, d_weights, log_mode, floor, _dp(d_out), out_frames, _VP(stream))
        _check(rc, self._ctx)

    def fbank_device(self, d_src, rows, channels, src_stride, frames, win_length, n_fft, hop, n_mels, d_window, d_basis, d_fb, flags,
                     preemphasis, scale, d_out, out_frames, stream=0):
        """alacgpu_fbank_device: Kaldi's fbank features of d_src (float32 device tensor, planar [rows, channels, src_stride], the
        first `frames` of a plane are signal) into d_out (float32 [rows, channels, n_mels, out_frames], out_frames as
        fbank.KaldiFbank.frames gives it, every element written) with the tables d_window [win_length], d_basis [win_length,
        2 * (n_fft // 2 + 1)] and d_fb [n_mels, n_fft // 2 + 1] (fbank.KaldiFbank builds them); flags: 1 snip_edges,
        2 remove_dc_offset, 4 use_power, 8 log.  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_fbank_device(self._ctx, _dp(d_src), rows, channels, src_stride, frames, win_length, n_fft, hop, n_mels,
                                        _dp(d_window), _dp(d_basis), _dp(d_fb), flags, preemphasis, scale, _dp(d_out), out_frames,
                                        _VP(stream))
        _check(rc, self._ctx)

    def mfcc_device(self, d_src, rows, channels, src_stride, frames, win_length, n_fft, hop, n_mels, n_ceps, d_window, d_basis, d_fb,
                    d_dct, d_lifter, flags, preemphasis, scale, energy_floor, d_out, out_frames, stream=0):
        """alacgpu_mfcc_device: Kaldi's MFCC features of d_src (float32 device tensor, planar [rows, channels, src_stride], the
        first `frames` of a plane are signal) into d_out (float32 [rows, channels, n_ceps, out_frames], out_frames as
        mfcc.KaldiMfcc.frames gives it, every element written) with fbank_device's three tables for n_mels filters, d_dct
        [n_ceps, n_mels] and d_lifter [n_ceps] (mfcc.KaldiMfcc builds them); flags: 1 snip_edges, 2 remove_dc_offset,
        4 use_power, 16 use_energy, 32 raw_energy.  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_mfcc_device(self._ctx, _dp(d_src), rows, channels, src_stride, frames, win_length, n_fft, hop, n_mels, n_ceps,
                                       _dp(d_window), _dp(d_basis), _dp(d_fb), _dp(d_dct), _dp(d_lifter), flags, preemphasis, scale,
                                       energy_floor, _dp(d_out), out_frames, _VP(stream))
        _check(rc, self._ctx)

    def deltas_device(self, d_src, d_out, rows, channels, n_feats, src_stride, out_stride, line_len, d_lengths, order, window, d_scales,
                      stream=0):
        """alacgpu_deltas_device: the features d_src (float32 device tensor [rows, channels, n_feats, src_stride], the first
        line_len of a line are frames) and their deltas of order 1 .. order into d_out (float32 [rows, channels,
        (order + 1) * n_feats, out_stride], apart from d_src) with the scales d_scales (deltas.Deltas builds them), the clamp of
        every order into the first len = min(max(d_lengths[row], 0), line_len) frames; zeros behind them.  d_lengths: an int64
        device tensor [rows], or None for line_len.  deltas.py states the arithmetic.  One launch, asynchronous on `stream`
        (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_deltas_device(self._ctx, _dp(d_src), _dp(d_out), rows, channels, n_feats, src_stride, out_stride, line_len,
                                         _dp(d_lengths), order, window, _dp(d_scales), _VP(stream))
        _check(rc, self._ctx)

    def normalize_meanvar_device(self, d_src, d_out, rows, lines_per_row, line_stride, line_len, d_valid, centre, scale, eps, stream=0):
        """alacgpu_normalize_meanvar_device: every line of d_src (float32 device tensor [rows, lines_per_row, line_stride], the
        first line_len of a line are data) to zero mean (centre) and unit variance (scale; eps under the root) over its first
        v = min(max(d_valid[row], 0), line_len) elements, zeros behind them up to line_len, into d_out (d_src itself or the
        same layout apart from it).  d_valid: an int64 device tensor [rows], or None for whole lines.  normalize.py states the
        arithmetic.  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_normalize_meanvar_device(self._ctx, _dp(d_src), _dp(d_out), rows, lines_per_row, line_stride, line_len,
                                                    _dp(d_valid), int(bool(centre)), int(bool(scale)), eps, _VP(stream))
        _check(rc, self._ctx)

    def normalize_top_device(self, d_src, d_out, rows, lines_per_row, line_stride, line_len, top, scale, offset, relative, stream=0):
        """alacgpu_normalize_top_device: with mx the maximum of row r of d_src (float32 device tensor
        [rows, lines_per_row, line_stride], the first line_len of a line are data), scale * (max(x, mx - top) [- mx with
        relative]) + offset into d_out (d_src itself or the same layout apart from it); a row with a NaN is NaN throughout.
        Two launches, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_normalize_top_device(self._ctx, _dp(d_src), _dp(d_out), rows, lines_per_row, line_stride, line_len, top,
                                                scale, offset, int(bool(relative)), _VP(stream))
        _check(rc, self._ctx)

    def normalize_sliding_device(self, d_src, d_out, rows, lines_per_row, line_stride, line_len, d_valid, window, min_window, center,
                                 norm_vars, stream=0):
        """alacgpu_normalize_sliding_device: Kaldi's sliding-window CMVN of every line of d_src (float32 device tensor
        [rows, lines_per_row, line_stride], the first line_len of a line are frames): frame t below v = min(max(d_valid[row],
        0), line_len) minus the mean of its window of `window` frames (around it with center, else behind it and at least
        min_window frames long at the start), divided by the window's standard deviation with norm_vars; zeros behind v up to
        line_len, into d_out (d_src itself or the same layout apart from it).  d_valid: an int64 device tensor [rows], or
        None for whole lines.  sliding.py states the arithmetic.  One launch, asynchronous on `stream` (raw hipStream_t);
        nothing is read back."""
        rc = lib().alacgpu_normalize_sliding_device(self._ctx, _dp(d_src), _dp(d_out), rows, lines_per_row, line_stride, line_len,
                                                    _dp(d_valid), window, min_window, int(bool(center)), int(bool(norm_vars)),
                                                    _VP(stream))
        _check(rc, self._ctx)

    def pcen_device(self, d_src, d_out, rows, lines_per_row, line_stride, line_len, d_valid, b, gain, bias, power, bias_pow, eps, scale,
                    d_table=None, lines_per_param=0, stage=0, stream=0):
        """alacgpu_pcen_device: per-channel energy normalisation of every line of d_src (float32 device tensor
        [rows, lines_per_row, line_stride], the first line_len of a line are frames) over its first v = min(max(d_valid[row],
        0), line_len) frames: s = scale * x, M the first-order smoothing of s with coefficient b from M[0] = s[0], and
        (s / (eps + M)^gain + bias)^power - bias_pow; zeros behind v up to line_len, into d_out (d_src itself or the same
        layout apart from it).  bias_pow: bias^power from float64.  d_table: None, or a float32 device tensor
        [5, lines_per_param] with b, gain, bias, power and bias^power of line % lines_per_param, in place of the five scalars.
        stage 1 writes M.  d_valid: an int64 device tensor [rows], or None for whole lines.  pcen.py states the arithmetic.
        One launch, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_pcen_device(self._ctx, _dp(d_src), _dp(d_out), rows, lines_per_row, line_stride, line_len, _dp(d_valid), b,
                                       gain, bias, power, bias_pow, eps, scale, _dp(d_table), lines_per_param, stage, _VP(stream))
        _check(rc, self._ctx)

    def vad_energy_device(self, d_src, rows, row_stride, line, line_len, d_valid, energy_threshold, energy_mean_scale, frames_context,
                          proportion_threshold, d_mask, mask_stride, stream=0):
        """alacgpu_vad_energy_device: Kaldi's energy VAD on the line_len floats at d_src + row * row_stride + line of every
        row (d_src: a float32 device tensor; row_stride and line in elements) over the first v = min(max(d_valid[row], 0),
        line_len) of them: frame t is voiced when at least proportion_threshold of the frames within frames_context of it
        are above energy_threshold + energy_mean_scale * their mean; the decisions, 0 at and behind v, into d_mask (uint8
        device tensor [rows, mask_stride]).  d_valid: an int64 device tensor [rows], or None for line_len.  vad.py states the
        arithmetic.  One launch, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_vad_energy_device(self._ctx, _dp(d_src), rows, row_stride, line, line_len, _dp(d_valid), energy_threshold,
                                             energy_mean_scale, frames_context, proportion_threshold, _dp(d_mask), mask_stride,
                                             _VP(stream))
        _check(rc, self._ctx)

    def select_frames_device(self, d_src, d_out, rows, lines_per_row, line_stride, line_len, d_valid, d_mask, mask_stride,
                             d_new_lengths, stream=0):
        """alacgpu_select_frames_device: every line of d_src (float32 device tensor [rows, lines_per_row, line_stride], the
        first line_len of a line are frames) keeps its frames t below v = min(max(d_valid[row], 0), line_len) with
        d_mask[row, t] != 0 (uint8 device tensor [rows, mask_stride]), in order, zeros behind them up to line_len, into d_out
        (d_src itself or the same layout apart from it); their number -- d_valid[row] itself where that is negative -- into
        d_new_lengths (int64 device tensor [rows]; may be d_valid).  d_valid: an int64 device tensor [rows], or None for
        line_len.  One launch, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_select_frames_device(self._ctx, _dp(d_src), _dp(d_out), rows, lines_per_row, line_stride, line_len,
                                                _dp(d_valid), _dp(d_mask), mask_stride, _dp(d_new_lengths), _VP(stream))
        _check(rc, self._ctx)

    def mix_device(self, d_src, d_out, d_noise, rows, channels, noise_channels, stride, noise_stride, frames, d_valid, d_noise_valid,
                   d_ratio, stream=0):
        """alacgpu_mix_device: y = x + g n, g = d_ratio[row] * sqrt(Ps / Pn), for every row of d_src (float32 device tensor,
        planar [rows, channels, stride], the first `frames` of a plane are data) and d_noise ([rows, noise_channels,
        noise_stride], noise_channels 1 or channels) over the first v = min(max(d_valid[row], 0), frames) frames, the noise's
        first vn repeated where vn < v, into d_out (d_src itself or the same layout apart from it).  d_valid, d_noise_valid:
        int64 device tensors [rows], or None for `frames`; d_ratio: float32 [rows], 0 for a row that gets no noise.  mix.py
        states the arithmetic.  Two launches, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_mix_device(self._ctx, _dp(d_src), _dp(d_out), _dp(d_noise), rows, channels, noise_channels, stride,
                                      noise_stride, frames, _dp(d_valid), _dp(d_noise_valid), _dp(d_ratio), _VP(stream))
        _check(rc, self._ctx)

    def biquad_device(self, d_src, d_out, rows, channels, stride, frames, d_valid, d_coeffs, sections, d_gain, clamp, stream=0):
        """alacgpu_biquad_device: every row of d_src (float32 device tensor, planar [rows, channels, stride], the first `frames`
        of a plane are data) through its cascade of `sections` biquad sections d_coeffs (float64 device tensor [rows, sections,
        5] = (b0, b1, b2, a1, a2)) and its gain d_gain (float64 [rows], or None for 1), over the first v = min(max(d_valid[row],
        0), frames) frames, limited to -1 .. 1 with clamp, into d_out (d_src itself or the same layout apart from it).  d_valid:
        an int64 device tensor [rows], or None for `frames`.  biquad.py states the arithmetic.  One launch, asynchronous on
        `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_biquad_device(self._ctx, _dp(d_src), _dp(d_out), rows, channels, stride, frames, _dp(d_valid),
                                         _dp(d_coeffs), sections, _dp(d_gain), int(bool(clamp)), _VP(stream))
        _check(rc, self._ctx)

    def level_device(self, d_src, d_out, rows, channels, stride, frames, d_valid, mode, hop, d_kweight, target, max_peak, clamp,
                     d_gain_out=None, d_energy_out=None, d_peak_out=None, stream=0):
        """alacgpu_level_device: every row of d_src (float32 device tensor, planar [rows, channels, stride], the first `frames`
        of a plane are data) brought to a level over its first v = min(max(d_valid[row], 0), frames) frames, into d_out (d_src
        itself, the same layout apart from it, or None: measured only).  mode 0, 1, 2: peak, RMS, BS.1770 loudness with hops of
        `hop` frames and the two K-weighting sections d_kweight (float64 device tensor [2, 5]; None for the other modes);
        target: linear (the peak, the mean square, 10^((LUFS + 0.691) / 10)); max_peak: the gain's limit, 0 for none; clamp:
        limited to -1 .. 1.  d_valid: an int64 device tensor [rows], or None for `frames`.  d_gain_out, d_energy_out, d_peak_out:
        float64 device tensors [rows] for the gain, the measured energy and the peak, or None.  level.py states the arithmetic.
        Two launches, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_level_device(self._ctx, _dp(d_src), _dp(d_out), rows, channels, stride, frames, _dp(d_valid), mode, hop,
                                        _dp(d_kweight), float(target), float(max_peak), int(bool(clamp)), _dp(d_gain_out),
                                        _dp(d_energy_out), _dp(d_peak_out), _VP(stream))
        _check(rc, self._ctx)

    def yin_device(self, d_src, rows, channels, stride, frames, d_valid, sample_rate, win_length, hop, tau_min, tau_max, align_length,
                   threshold, d_out, out_frames, stream=0):
        """alacgpu_yin_device: the YIN F0 estimate of every frame of every row of d_src (float32 device tensor, planar [rows,
        channels, stride], the first `frames` of a plane are data) over its first v = min(max(d_valid[row], 0), frames) samples,
        into d_out (float32 device tensor [rows, channels, 2, out_frames]: f0 in Hz, the aperiodicity; zeros behind a row's
        frames).  d_valid: an int64 device tensor [rows], or None for `frames`.  align_length 0: centred frames.  yin.py states
        the arithmetic.  One launch, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_yin_device(self._ctx, _dp(d_src), rows, channels, stride, frames, _dp(d_valid), sample_rate, win_length, hop,
                                      tau_min, tau_max, align_length, float(threshold), _dp(d_out), out_frames, _VP(stream))
        _check(rc, self._ctx)

    def pyin_device(self, d_src, rows, channels, stride, frames, d_valid, sample_rate, win_length, hop, tau_min, tau_max, align_length,
                    n_thresholds, n_bins, band, no_trough_prob, d_table, d_obs_voiced, d_obs_unvoiced, d_vp, d_out, d_states, out_frames,
                    stage=0, stream=0):
        """alacgpu_pyin_device: probabilistic YIN on every row of d_src (float32 device tensor, planar [rows, channels, stride],
        framed as `yin_device` frames it) with the packed float32 tables d_table of a pyin.PYin.  stage 0: both launches, into
        d_out (float32 [rows, channels, 3, out_frames]: the decoded bin's frequency, 1 where voiced, the voicing probability;
        zeros behind a row's frames), the observations and backpointers in the context's scratch; stage 1: the observations
        alone into d_obs_voiced [rows, channels, out_frames, n_bins], d_obs_unvoiced and d_vp [rows, channels, out_frames];
        stage 2: the decode alone on d_obs_voiced and d_obs_unvoiced into d_states (int32 [rows, channels, out_frames], -1
        behind a row's frames), d_valid then counting frames.  Tensors a stage does not use are None.  pyin.py states the
        arithmetic.  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_pyin_device(self._ctx, _dp(d_src), rows, channels, stride, frames, _dp(d_valid), sample_rate, win_length, hop,
                                       tau_min, tau_max, align_length, n_thresholds, n_bins, band, float(no_trough_prob), _dp(d_table),
                                       _dp(d_obs_voiced), _dp(d_obs_unvoiced), _dp(d_vp), _dp(d_out), _dp(d_states), out_frames, int(stage),
                                       _VP(stream))
        _check(rc, self._ctx)

    def kaldi_pitch_device(self, d_src, rows, channels, stride, frames, d_valid, sample_rate, resample_freq, win_length, hop, window, shift,
                           first_lag, last_lag, n_states, phases, in_per_unit, down_taps, up_taps, flags, left_context, right_context,
                           delta_window, d_table, d_nccf, d_raw, d_out, out_frames, stage=0, stream=0):
        """alacgpu_kaldi_pitch_device: Kaldi's pitch features of every row of d_src (float32 device tensor, planar [rows, channels,
        stride]) with the packed float32 tables d_table of a kaldi_pitch.KaldiPitch.  stage 0: all three launches, into d_out
        (float32 [rows, channels, lines, out_frames]; zeros behind a row's frames), the NCCF planes and backpointers in the
        context's scratch; stage 1: the downsampler and the NCCF alone into d_nccf [rows, channels, 2, out_frames, n_states];
        stage 2: the decode alone on d_nccf into d_raw [rows, channels, 2, out_frames]; stage 3: the post-processing alone on
        d_raw into d_out; in stages 2 and 3 d_valid counts frames.  Tensors a stage does not use are None.  kaldi_pitch.py states
        the arithmetic.  Asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_kaldi_pitch_device(self._ctx, _dp(d_src), rows, channels, stride, frames, _dp(d_valid), sample_rate, resample_freq,
                                              win_length, hop, window, shift, first_lag, last_lag, n_states, phases, in_per_unit, down_taps,
                                              up_taps, flags, left_context, right_context, delta_window, _dp(d_table), _dp(d_nccf),
                                              _dp(d_raw), _dp(d_out), out_frames, int(stage), _VP(stream))
        _check(rc, self._ctx)

    def reverb_device(self, d_src, d_out, d_rir, rows, channels, rir_channels, stride, rir_stride, frames, rir_frames, d_valid,
                      d_rir_valid, stream=0):
        """alacgpu_reverb_device: every row of d_src (float32 device tensor, planar [rows, channels, stride], the first `frames`
        of a plane are data) convolved with its impulse response in d_rir ([rows, rir_channels, rir_stride], rir_channels 1 or
        channels, the first `rir_frames` are data), aligned on the response's direct path and scaled to unit energy, over the
        first v = min(max(d_valid[row], 0), frames) frames, into d_out (d_src itself or the same layout apart from it).
        d_valid, d_rir_valid: int64 device tensors [rows], or None for all; a row whose d_rir_valid is 0 stays as it is.
        reverb.py states the arithmetic.  Two launches, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_reverb_device(self._ctx, _dp(d_src), _dp(d_out), _dp(d_rir), rows, channels, rir_channels, stride,
                                         rir_stride, frames, rir_frames, _dp(d_valid), _dp(d_rir_valid), _VP(stream))
        _check(rc, self._ctx)

    def rir_shoebox_device(self, d_geometry, d_beta, rows, sample_rate, frames, taps, max_order, sound_speed, d_out, out_stride,
                           d_lengths, stream=0):
        """alacgpu_rir_shoebox_device: the image-source response of every row's room (d_geometry float64 device tensor
        [rows, 9], d_beta float32 [rows, 6]) into the first `frames` of every row of d_out (float32 [rows, out_stride]) and its
        length -- frames, or 0 where the row is refused -- into d_lengths (int32 [rows]).  max_order -1: every order.  rir.py
        states the arithmetic.  One launch, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_rir_shoebox_device(self._ctx, _dp(d_geometry), _dp(d_beta), rows, sample_rate, frames, taps, max_order,
                                              float(sound_speed), _dp(d_out), out_stride, _dp(d_lengths), _VP(stream))
        _check(rc, self._ctx)

    def time_stretch_device(self, d_src, d_out, rows, channels, src_stride, out_stride, frames, out_frames, d_p, d_q, d_valid,
                            d_valid_out, n_fft, stream=0):
        """alacgpu_time_stretch_device: every row of d_src (float32 device tensor, planar [rows, channels, src_stride], the
        first `frames` of a plane are data) stretched by d_p[row] / d_q[row] (int32 device tensors [rows]) over its first
        v = min(max(d_valid[row], 0), frames) frames with the pitch kept, into d_out ([rows, channels, out_stride] apart from
        it, of which the first out_frames are written: (2 v p + q) div (2 q) frames and zeros behind them); the new lengths
        into d_valid_out (int64 device tensor [rows]).  A row with p == q or at most n_fft / 2 valid frames is neither read
        nor written.  d_valid: an int64 device tensor [rows], or None for `frames`.  n_fft: 512, 1024 or 2048.  pitch.py states
        the arithmetic.  Three launches, asynchronous on `stream` (raw hipStream_t); nothing is read back."""
        rc = lib().alacgpu_time_stretch_device(self._ctx, _dp(d_src), _dp(d_out), rows, channels, src_stride, out_stride, frames,
                                               out_frames, _dp(d_p), _dp(d_q), _dp(d_valid), _dp(d_valid_out), n_fft, _VP(stream))
        _check(rc, self._ctx)

    def copy_rows_device(self, d_src, d_out, rows, channels, src_stride, out_stride, frames, d_valid, stream=0):
        """alacgpu_copy_rows_device: the first min(max(d_valid[row], 0), frames) frames of every plane of d_src (float32
        device tensor [rows, channels, src_stride]) into d_out ([rows, channels, out_stride], apart from it); nothing else is
        written.  d_valid: an int64 device tensor [rows].  One launch, asynchronous on `stream` (raw hipStream_t)."""
        rc = lib().alacgpu_copy_rows_device(self._ctx, _dp(d_src), _dp(d_out), rows, channels, src_stride, out_stride, frames,
                                            _dp(d_valid), _VP(stream))
        _check(rc, self._ctx)

    def specaugment_device(self, d_src, d_out, rows, channels, n_mels, line_stride, line_len, d_valid, d_warp, d_freq, d_time, fill,
                           stream=0):
        """alacgpu_specaugment_device: SpecAugment on d_src (float32 device tensor [rows, channels, n_mels, line_stride], the
        first line_len of a line are frames) into d_out (d_src itself or the same layout apart from it), over the first
        tau = min(max(d_valid[row], 0), line_len) frames of every row: the time warp d_warp (int32 device tensor [rows, 2] of
        (c, c'), or None), then the frequency masks d_freq [rows, n_freq, 2] and the time masks d_time [rows, n_time, 2]
        (int32, (first, width); None for none) set to `fill`.  d_valid: an int64 device tensor [rows], or None for whole
        lines.  augment.py states the arithmetic.  One launch, asynchronous on `stream` (raw hipStream_t); nothing is read
        back."""
        rc = lib().alacgpu_specaugment_device(self._ctx, _dp(d_src), _dp(d_out), rows, channels, n_mels, line_stride, line_len,
                                              _dp(d_valid), _dp(d_warp), _dp(d_freq), 0 if d_freq is None else d_freq.shape[1],
                                              _dp(d_time), 0 if d_time is None else d_time.shape[1], fill, _VP(stream))
        _check(rc, self._ctx)

    def set_output_format(self, fmt):
        """0: int32 per sample (default).  1: packed little-endian PCM bytes (FormatSamples fused into the store);
        packet p's bytes are pcm[p].view(uint8)[:out_bytes[p]]."""
        _check(lib().alacgpu_set_output_format(self._ctx, fmt), self._ctx)

    def set_pairing(self, on):
        """Pairing (include/alacgpu.h): decode_batch_device on up to 4096 resident packets it has decoded before takes both
        channels of a packet in one pass, from a remembered and verified start of channel B.  On by default."""
        _check(lib().alacgpu_set_pairing(self._ctx, int(bool(on))), self._ctx)

    def pairing_stats(self):
        """(paired, missed, wrong): packets decoded paired, two-channel packets without a remembered start, packets whose
        remembered start was wrong, since the context was made.  Waits for the device."""
        out = np.zeros(3, dtype=np.uint64)
        _check(lib().alacgpu_pairing_stats(self._ctx, _ptr(out)), self._ctx)
        return tuple(int(v) for v in out)

    def pairing_shift_starts(self):
        """For tests of the check: every remembered start one bit on.  Waits for the device."""
        _check(lib().alacgpu_pairing_shift_starts(self._ctx), self._ctx)

    def last_kernel_ms(self):
        return float(lib().alacgpu_last_kernel_ms(self._ctx))

    def decode_frame(self, cfg_index, packet):
        """Single-packet DecodeFrame in the reference's own int[] layout.
        Returns (ref_ints, out_bytes, status)."""
        pkt = np.frombuffer(bytes(packet), dtype=np.uint8)
        cfg = self.cfgs[cfg_index]
        cap = MAX_FRAME * int(cfg["num_channels"]) * (3 if int(cfg["sample_size"]) == 24 else 1)
        out = np.zeros(cap, dtype=np.int32)
        ob = C.c_int32(0)
        st = C.c_int32(0)
        rc = lib().alacgpu_decode_frame(self._ctx, cfg_index, _ptr(pkt), len(pkt), _ptr(out), cap, C.byref(ob),
                                        C.byref(st))
        _check(rc, self._ctx)
        return out, ob.value, st.value


def shard_ranges(sizes, world):
    """alacgpu_shard_ranges: the packet partition of every multi-GPU entry point -- contiguous ranges cut at multiples of 8
    packets, balanced by packet bytes.  Returns first[world + 1]; rank r owns packets first[r] .. first[r+1].  Host arithmetic."""
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    first = np.zeros(world + 1, dtype=np.uint32)
    _check(lib().alacgpu_shard_ranges(_ptr(sizes), len(sizes), world, _ptr(first)))
    return first


class AlacGpuComm(_Closing):
    """alacgpu_comm: this rank's handle on the RCCL communicator for the all-gather of decoded PCM (one process per GPU).
    `unique_id()` on rank 0, hand the 128 bytes to the other ranks (torch.distributed broadcast, a file, MPI ...), then
    every rank constructs AlacGpuComm(ctx, id, rank, world) -- a collective call."""

    @staticmethod
    def unique_id():
        buf = np.zeros(128, dtype=np.uint8)
        _check_comm(lib().alacgpu_comm_get_unique_id(_ptr(buf)), None)
        return buf

    def __init__(self, ctx, unique_id, rank, world):
        self._comm = _VP()
        self.ctx, self.rank, self.world = ctx, rank, world
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        rc = lib().alacgpu_comm_create(ctx._ctx, _ptr(uid), rank, world, C.byref(self._comm))
        if rc != 0:
            self._comm = _VP()
        _check_comm(rc, None)

    def allgather_pcm(self, d_full, first, slot_ints, stream=0):
        """d_full: torch int32 CUDA tensor [n_packets, slot_ints] holding this rank's packets first[rank]..first[rank+1]
        decoded in place; asynchronous on `stream` (raw hipStream_t)."""
        first = np.ascontiguousarray(first, dtype=np.uint32)
        _check_comm(lib().alacgpu_allgather_pcm(self._comm, _dp(d_full), _ptr(first), slot_ints, _VP(stream)), self._comm)

    def decode_allgather_device(self, d_blob, blob_bytes, d_offsets, d_sizes, d_cfg_idx, first, d_full, slot_ints, d_out_bytes,
                                d_out_samples, d_status, n_chunks=4, stream=0):
        """Decode this rank's range (device arrays indexed by GLOBAL packet number) in n_chunks pieces and gather piece k
        while piece k+1 decodes; asynchronous on `stream`."""
        first = np.ascontiguousarray(first, dtype=np.uint32)
        _check_comm(lib().alacgpu_decode_allgather_device(self.ctx._ctx, self._comm, _dp(d_blob), blob_bytes, _dp(d_offsets),
                                                          _dp(d_sizes), _dp(d_cfg_idx), _ptr(first), _dp(d_full), slot_ints,
                                                          _dp(d_out_bytes), _dp(d_out_samples), _dp(d_status), n_chunks,
                                                          _VP(stream)), self._comm)

    def close(self):
        if self._comm:
            lib().alacgpu_comm_destroy(self._comm)
            self._comm = _VP()


def decode_batch_sharded(contexts, blob, offsets, sizes, cfg_idx=None, slot_ints=None, out=None):
    """alacgpu_decode_batch_sharded: one host batch over several AlacGpuContext objects (one per GPU) from this process.
    Returns (pcm[n, slot_ints] int32, out_bytes[n], out_samples[n], status[n]) like AlacGpuContext.decode_batch."""
    args, outs = _host_batch(contexts[0].cfgs, blob, offsets, sizes, cfg_idx, slot_ints, out)
    handles = (_VP * len(contexts))(*[c._ctx for c in contexts])
    _check(lib().alacgpu_decode_batch_sharded(handles, len(contexts), *args), contexts[0]._ctx)
    return outs


class PinnedBuffer(_Closing):
    """Page-locked host memory from alacgpu_alloc_pinned, viewed as a numpy array (batch buffers that are reused across
    calls: transfers from and to it run at link speed).  Free with close() / as a context manager."""

    def __init__(self, shape, dtype):
        self._shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self._dtype = np.dtype(dtype)
        nbytes = int(np.prod(self._shape, dtype=np.int64)) * self._dtype.itemsize
        self._p = lib().alacgpu_alloc_pinned(max(nbytes, 1))
        if not self._p:
            raise AlacGpuError("alacgpu_alloc_pinned failed")
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=self._dtype, count=int(np.prod(self._shape, dtype=np.int64))).reshape(self._shape)

    def close(self):
        if self._p:
            self.array = None
            lib().alacgpu_free_pinned(self._p)
            self._p = None


def device_count():
    """Usable gfx950 devices (0: none -- creating a context then fails, there is no CPU fallback)."""
    return int(lib().alacgpu_device_count())


def expand_reference_layout(cfg_row, pcm, n_samples):
    cfgs = make_cfgs([cfg_row]) if not isinstance(cfg_row, np.ndarray) else cfg_row
    nc = int(cfgs[0]["num_channels"])
    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
    out = np.zeros(n_samples * nc * 3 + 8, dtype=np.int32)
    cnt = lib().alacgpu_expand_reference_layout(_ptr(cfgs), _ptr(pcm), n_samples, _ptr(out))
    return out[:cnt].copy()


def format_samples(bps, ref_ints, count_bytes):
    """AlacContext.FormatSamples (AlacContext.cs:214-256)."""
    ref_ints = np.ascontiguousarray(ref_ints, dtype=np.int32)
    dst = np.zeros(max(count_bytes, 0) + 8, dtype=np.uint8)
    cnt = lib().alacgpu_format_samples(bps, _ptr(ref_ints), count_bytes, _ptr(dst))
    return dst[:cnt].copy()


def cfg_from_codec_data(codec_data_ints, samplesize, numchannels):
    """AlacFile.SetInfo's parse (AlacFile.cs:63-93) of the int-per-byte CodecData array."""
    arr = np.ascontiguousarray(codec_data_ints, dtype=np.int32)
    cfg = np.zeros(1, dtype=CFG_DTYPE)
    _check(lib().alacgpu_cfg_from_codec_data(_ptr(arr), len(arr), samplesize, numchannels, _ptr(cfg)))
    return cfg


# ---- whole files into one tensor (alacgpu_decode_into_device) ------------------------------------------------------------
def _torch_dtype(torch, dtype):
    if dtype not in (torch.float32, torch.int32):
        raise ValueError(f"dtype must be torch.float32 or torch.int32, not {dtype}")
    return dtype


def _normalise_status(st, first_bytes):
    """AlacContext.ReadBatch's reading of the statuses: a one-channel element with a prediction type other than 0 is an ordinary
    packet (its un-predicted residuals, AlacFile.cs:484-496), an unsupported element a run of zeros (the reference decodes
    nothing, AlacFile.cs:437)."""
    mono = (first_bytes >> 5) == 0
    st = np.where((st == ST_UNSUPPORTED_PREDTYPE) & mono, ST_OK, st)
    return np.where(st == ST_UNSUPPORTED_ELEMENT, ST_OK, st)


def window_plan(dst_first, durations, offset, length):
    """The packets of frames offset .. offset + length of one file, on the host.  Frame t belongs to the packet p with
    dst_first[p] <= t < dst_first[p] + durations[p] (dst_first: the exclusive prefix sum of the durations, as packet_table
    gives them).  Returns (p0, p1, first, frames, skip): the contiguous packet range p0 .. p1 that overlaps the window (a
    window from frame 0 starts at packet 0; packets with no frames inside it are taken only between others), and per packet
    of it the run's first frame relative to the window, its frame count and the frames skipped at the packet's start
    (int64 arrays of p1 - p0).  A window of length 0 has no packets."""
    dst_first = np.asarray(dst_first, dtype=np.int64)
    durations = np.asarray(durations, dtype=np.int64)
    offset, length = int(offset), int(length)
    if offset < 0 or length < 0:
        raise ValueError(f"offset {offset} and length {length} must not be negative")
    end = offset + length
    if length == 0:
        p0 = p1 = 0
    else:
        p0 = 0 if offset == 0 else int(np.searchsorted(dst_first + durations, offset, side="right"))
        p1 = max(int(np.searchsorted(dst_first, end, side="left")), p0)
    f, d = dst_first[p0:p1], durations[p0:p1]
    lo = np.maximum(f, offset)
    frames = np.maximum(np.minimum(f + d, end) - lo, 0)
    return p0, p1, lo - offset, frames, lo - f


def _decode_tables(tables, cfgs, cfg_idx, ranges, dst_first, dst_frames, src_skip, out, channels, layout, plane_stride, device):
    """One alacgpu_decode_window_into_device call over the packets ranges[f] = (p0, p1) of every table (only their bytes are
    uploaded); src_skip None: no skip.  Returns the statuses and the packets' first bytes (host)."""
    import torch

    dev = torch.device("cuda", device)
    blobs, offs, sizes, firsts = [], [], [], []
    base = 0
    for t, (p0, p1) in zip(tables, ranges):
        o, z = t["offsets"][p0:p1], t["sizes"][p0:p1]
        start = int(o[0]) if len(o) else 0
        used = int(o[-1]) + int(z[-1]) - start if len(o) else 0   # (the range's bytes: nothing in front of or behind it)
        blobs.append(t["blob"][start:start + used])
        offs.append(o.astype(np.uint64) - np.uint64(start) + np.uint64(base))
        sizes.append(z)
        firsts.append(t["blob"][start + np.minimum(o - np.uint64(start), max(used - 1, 0)).astype(np.int64)] if used
                      else np.zeros(len(o), np.uint8))
        base += used
    offsets = np.concatenate(offs) if offs else np.zeros(0, np.uint64)
    n = len(offsets)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8)
    blob = np.zeros(base + 64, dtype=np.uint8)          # readable up to blob_bytes rounded up to 16
    blob[:base] = np.concatenate(blobs)
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_sz = torch.from_numpy(np.concatenate(sizes).astype(np.int32)).to(dev)
    d_ci = torch.from_numpy(cfg_idx.astype(np.int16)).to(dev)
    d_first = torch.from_numpy(dst_first.astype(np.int64)).to(dev)
    d_frames = torch.from_numpy(dst_frames.astype(np.int32)).to(dev)
    # a packet decodes at most 16384 frames: a window that starts further into it (a stts duration above 16384) is frames
    # that are zeros in the whole file too -- skip 16384 gives exactly those zeros, and the packet is still decoded and checked
    d_skip = (torch.from_numpy(np.minimum(src_skip, MAX_FRAME).astype(np.int32)).to(dev) if src_skip is not None else None)
    d_st = torch.empty(n, dtype=torch.int32, device=dev)
    with AlacGpuContext(cfgs, device) as ctx:
        stream = torch.cuda.current_stream(dev)
        ctx.decode_window_into_device(d_blob, base, d_off, d_sz, d_ci, n, d_first, d_frames, d_skip, out, channels, layout,
                                      plane_stride, None, d_st, stream=stream.cuda_stream)
        st = d_st.cpu().numpy()     # (waits for the decode: the context's scratch is released behind it)
    return st, np.concatenate(firsts)


def _frame_count(name, value, minimum=0):
    """An int argument (numpy ints too) that is at least `minimum`, else ValueError."""
    try:
        v = operator.index(value)
    except TypeError:
        raise ValueError(f"{name} must be an integer, not {value!r}") from None
    if v < minimum:
        raise ValueError(f"{name} must be at least {minimum}, not {v}")
    return v


def info(source):
    """The stream facts of an M4A file from its headers alone (no packet bytes, no GPU context): a dict with num_frames
    (AlacContext.GetNumSamples: the sum of the stts durations -- what `load` returns, and the frame offsets `load` and
    `load_batch` accept are 0 .. num_frames), channels, sample_rate and sample_size.  `source` as for `load`."""
    from .container import header_table

    h = header_table(source)
    return dict(num_frames=h["num_samples"], channels=h["num_channels"], sample_rate=h["sample_rate"],
                sample_size=h["sample_size"])


def load(source, device=0, dtype=None, layout="planar", frame_offset=0, num_frames=None):
    """Decode an M4A file on the GPU into one gap-free tensor: returns (pcm, sample_rate), pcm [C, n] (planar) or [n, C]
    (interleaved) on cuda:`device`.  float32 (default): sample * 2^-(bits-1), exact; int32: the canonical sample.  `source`:
    file bytes, a path, or a seekable binary file object.  frame_offset / num_frames: the window of frames frame_offset ..
    frame_offset + n, n = min(num_frames, T - frame_offset) (T = AlacContext.GetNumSamples(); num_frames None: to the end);
    only the packets that overlap it are uploaded and decoded.  ValueError (before any device work) for a frame_offset outside
    0 .. T or a negative num_frames.  Raises AlacGpuError naming the first packet (its index in the file) that does not decode
    (statuses read as AlacContext.ReadBatch reads them)."""
    import torch

    from .container import packet_table

    dtype = _torch_dtype(torch, torch.float32 if dtype is None else dtype)
    if layout not in ("planar", "interleaved"):
        raise ValueError(f"layout must be 'planar' or 'interleaved', not {layout!r}")
    frame_offset = _frame_count("frame_offset", frame_offset)
    if num_frames is not None:
        num_frames = _frame_count("num_frames", num_frames)
    t = packet_table(source)
    C_, T = int(t["num_channels"]), int(t["num_samples"])
    if frame_offset > T:
        raise ValueError(f"frame_offset {frame_offset} outside 0 .. {T}")
    L = T - frame_offset if num_frames is None else min(num_frames, T - frame_offset)
    if frame_offset == 0 and L == T:       # the whole file: every packet, as it always was
        p0, p1, first, frames, skip = 0, len(t["sizes"]), t["dst_first"], t["durations"], None
    else:
        p0, p1, first, frames, skip = window_plan(t["dst_first"], t["durations"], frame_offset, L)
    shape = (C_, L) if layout == "planar" else (L, C_)
    out = torch.zeros(shape, dtype=dtype, device=torch.device("cuda", device))
    st, first_bytes = _decode_tables([t], t["cfg"], np.zeros(p1 - p0, np.uint16), [(p0, p1)], first, frames,
                                     skip if skip is not None and skip.any() else None, out, C_, layout, max(L, 1), device)
    bad = np.nonzero(_normalise_status(st, first_bytes) != ST_OK)[0]
    if len(bad):
        p = int(bad[0])
        raise AlacGpuError(f"packet {p0 + p} does not decode: {_status_text(st[p])}")
    return out, int(t["sample_rate"])


def load_batch(sources, device=0, dtype=None, max_frames=None, frame_offsets=None):
    """Decode several M4A files in ONE launch into a zero-padded [F, C, Tmax] tensor: returns (pcm, lengths[F], sample_rate)
    (lengths: int64, host).  Files may mix 16- and 24-bit; they must share channel count and sample rate (ValueError).
    frame_offsets: an int or one per file (default 0): file f's window starts there, and lengths[f] = T_f - frame_offsets[f].
    max_frames: crop every window to at most that many frames.  Only the packets that overlap a window are uploaded and
    decoded.  ValueError (before any device work) for an offset outside 0 .. T_f or a frame_offsets of another length."""
    import torch

    from .container import packet_table

    dtype = _torch_dtype(torch, torch.float32 if dtype is None else dtype)
    tables = [packet_table(s) for s in sources]
    if not tables:
        raise ValueError("no sources")
    if len(tables) > 65536:
        raise ValueError("at most 65536 files per batch (one stream cfg each)")
    C_, rate = int(tables[0]["num_channels"]), int(tables[0]["sample_rate"])
    for i, t in enumerate(tables):
        if int(t["num_channels"]) != C_ or int(t["sample_rate"]) != rate:
            raise ValueError(f"source {i}: {t['num_channels']} channels at {t['sample_rate']} Hz, the first has {C_} at {rate} Hz")
    F = len(tables)
    totals = np.array([t["num_samples"] for t in tables], dtype=np.int64)
    if frame_offsets is None:
        offsets = np.zeros(F, dtype=np.int64)
    elif np.ndim(frame_offsets) == 0:
        offsets = np.full(F, _frame_count("frame_offsets", frame_offsets), dtype=np.int64)
    else:
        offsets = np.array([_frame_count(f"frame_offsets[{f}]", o) for f, o in enumerate(frame_offsets)], dtype=np.int64)
        if len(offsets) != F:
            raise ValueError(f"{len(offsets)} frame offsets for {F} sources")
    past = np.nonzero(offsets > totals)[0]
    if len(past):
        f = int(past[0])
        raise ValueError(f"source {f}: frame offset {offsets[f]} outside 0 .. {totals[f]}")
    lengths = totals - offsets
    if max_frames is not None:
        lengths = np.minimum(lengths, max(int(max_frames), 0))
    Tmax = int(lengths.max())
    out = torch.zeros((F, C_, Tmax), dtype=dtype, device=torch.device("cuda", device))
    ranges, ci, pk, firsts, frames, skips = [], [], [], [], [], []
    for f, t in enumerate(tables):
        p0, p1, first, fr, skip = window_plan(t["dst_first"], t["durations"], offsets[f], lengths[f])
        ranges.append((p0, p1))
        ci.append(np.full(p1 - p0, f, dtype=np.uint16))
        pk.append(np.arange(p0, p1))
        firsts.append(first + f * C_ * Tmax)
        frames.append(fr)
        skips.append(skip)
    cfgs = np.concatenate([t["cfg"] for t in tables])
    skip = np.concatenate(skips)
    st, first_bytes = _decode_tables(tables, cfgs, np.concatenate(ci), ranges, np.concatenate(firsts), np.concatenate(frames),
                                     skip if skip.any() else None, out, C_, "planar", max(Tmax, 1), device)
    bad = np.nonzero(_normalise_status(st, first_bytes) != ST_OK)[0]
    if len(bad):
        p = int(bad[0])
        f, q = int(np.concatenate(ci)[p]), int(np.concatenate(pk)[p])
        raise AlacGpuError(f"source {f}, packet {q} does not decode: {_status_text(st[p])}")
    return out, torch.from_numpy(lengths), rate


# ---- tensors to M4A files (alacgpu_encode_device) -----------------------------------------------------------------------------
def encode_max_packet_bytes(frames, sample_size, channels):
    """alacgpu_encode_max_packet_bytes: the largest packet the encoder writes for that many frames (an escape packet with its
    sample count and the END tag, rounded up to 16 bytes)."""
    return int(lib().alacgpu_encode_max_packet_bytes(int(frames), int(sample_size), int(channels)))


def _check_save_args(pcm, batch, sample_size, frame_length, sample_rate):
    """The host-side checks of save / save_batch, before any device work; returns (F, C, T)."""
    import torch

    want = 3 if batch else 2
    if not isinstance(pcm, torch.Tensor) or pcm.dim() != want:
        raise ValueError(f"pcm must be a torch tensor of shape {'[F, C, T]' if batch else '[C, T]'}")
    F, C_, T = (pcm.shape[0], pcm.shape[1], pcm.shape[2]) if batch else (1, pcm.shape[0], pcm.shape[1])
    if C_ not in (1, 2):
        raise ValueError(f"{C_} channels: ALAC here is one or two channels")
    if pcm.dtype not in (torch.int32, torch.float32):
        raise ValueError(f"pcm must be torch.int32 or torch.float32, not {pcm.dtype}")
    if sample_size not in (16, 24):
        raise ValueError(f"sample_size must be 16 or 24, not {sample_size}")
    if not isinstance(frame_length, (int, np.integer)) or not 1 <= int(frame_length) <= MAX_FRAME:
        raise ValueError(f"frame_length must be 1 .. {MAX_FRAME}, not {frame_length}")
    if not isinstance(sample_rate, (int, np.integer)) or not 1 <= int(sample_rate) < 1 << 32:
        raise ValueError(f"sample_rate must be a positive 32-bit integer, not {sample_rate}")
    if F == 0 or T == 0:
        raise ValueError("empty input: nothing to encode")
    return F, C_, T


def _check_stco(T, C_, sample_size, frame_length):
    """A file's 32-bit chunk offsets must hold its media data at its worst case (every packet an escape packet)."""
    n = -(-int(T) // int(frame_length))
    worst = n * encode_max_packet_bytes(frame_length, sample_size, C_) + 64 * n + 4096   # packets, the tables, the atoms
    if worst >= 1 << 32:
        raise ValueError(f"{T} frames can need {worst} bytes: more than the 32-bit chunk offsets (stco) of an M4A file address")


class _Encoded:
    """What _encode_slots leaves behind: the batch's packet list (host) and the encoder's slot buffer, sizes and statuses
    (device)."""


def _encode_slots(ctx, pcm, lengths, frame_length, stream):
    """The packet list of pcm[F, C, T] (frames 0 .. lengths[f] of every file, frame_length frames per packet, a shorter last
    one) and ONE alacgpu_encode_device call over it with cfg 0 of `ctx` on `stream` (raw hipStream_t), into a fresh slot
    buffer.  Nothing is read back."""
    import torch

    F, C_, T = pcm.shape
    dev = pcm.device
    e = _Encoded()
    e.counts = [-(-int(L) // frame_length) for L in lengths]
    e.file_of = np.repeat(np.arange(F, dtype=np.int64), e.counts)
    first_in_file = np.concatenate([np.arange(c, dtype=np.int64) * frame_length for c in e.counts])
    e.frames = np.minimum(np.repeat(np.asarray(lengths, dtype=np.int64), e.counts) - first_in_file, frame_length)
    n = e.n = len(e.file_of)
    e.slot = encode_max_packet_bytes(frame_length, int(ctx.cfgs[0]["sample_size"]), C_)
    d_first = torch.from_numpy(e.file_of * C_ * T + first_in_file).to(dev)
    d_frames = torch.from_numpy(e.frames.astype(np.int32)).to(dev)
    d_ci = torch.zeros(n, dtype=torch.int16, device=dev)
    e.d_packets = torch.empty(n * e.slot, dtype=torch.uint8, device=dev)
    e.d_sizes = torch.zeros(n, dtype=torch.int32, device=dev)
    e.d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx.encode_device(pcm.contiguous(), C_, d_first, d_frames, d_ci, n, e.d_packets, e.slot, e.d_sizes, e.d_st, layout="planar",
                      plane_stride=T, stream=stream)
    return e


def _compact_slots(ctx, e, d_blob, base, capacity, d_pkt_offset, stream):
    """One alacgpu_compact_packets_device call over the slots of `e` behind its encode, and the ONE small read: returns (the
    packets' bytes in all, the first packet whose status is not ALACGPU_ST_OK or e.n), both reduced on the device."""
    import torch

    dev = e.d_sizes.device
    d_total = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.compact_packets_device(e.d_packets, e.slot, e.d_sizes, e.n, d_blob, base, capacity, d_pkt_offset, d_total, stream=stream)
    bad = torch.where(e.d_st != ST_OK, torch.arange(e.n, dtype=torch.int64, device=dev), e.n).min()
    total, bad = (int(x) for x in torch.stack([d_total[0], bad]).cpu())
    return total, bad


def _encode_tensor(pcm, lengths, sample_size, frame_length, device):
    """One alacgpu_encode_device call over every file of pcm[F, C, T] (frames 0 .. lengths[f]); returns per file the list of
    packet bytes.  Only the packets' own bytes are copied to the host: they are compacted on the device first
    (alacgpu_compact_packets_device: once without room, for the size, then into exactly that many bytes)."""
    import torch

    F, C_, T = pcm.shape
    dev = pcm.device
    with AlacGpuContext([(frame_length, sample_size, 40, 10, 14, C_)], device) as ctx:
        stream = torch.cuda.current_stream(dev).cuda_stream
        e = _encode_slots(ctx, pcm, lengths, frame_length, stream)
        d_off = torch.empty(e.n, dtype=torch.int64, device=dev)
        d_blob = torch.empty(16, dtype=torch.uint8, device=dev)
        total, bad = _compact_slots(ctx, e, d_blob, 0, 0, d_off, stream)
        if bad < e.n:
            raise AlacGpuError(f"packet {bad} was not encoded: {_status_text(int(e.d_st[bad]))}")
        d_blob = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        _compact_slots(ctx, e, d_blob, 0, total, d_off, stream)   # (its read waits for the copy: the context may go)
    blob = d_blob[:total].cpu().numpy().tobytes()
    sizes = e.d_sizes.cpu().numpy().astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    out, p = [], 0
    for f in range(F):
        out.append([blob[offs[q]:offs[q + 1]] for q in range(p, p + e.counts[f])])
        p += e.counts[f]
    return out, [e.frames[e.file_of == f] for f in range(F)]


def _write_file(dest, packets, durations, frame_length, sample_size, channels, sample_rate, rice=(40, 10, 14)):
    from .container import write_m4a

    sizes = [len(x) for x in packets]
    frames = int(np.sum(durations))
    seconds = frames / float(sample_rate)
    avg = int(round(8 * sum(sizes) / seconds)) if seconds > 0 else 0
    data = write_m4a(packets, [int(d) for d in durations], frame_len=frame_length, sample_size=sample_size, channels=channels,
                     sample_rate=sample_rate, pb=rice[0], mb=rice[1], kb=rice[2], max_frame_bytes=max(sizes),
                     avg_bitrate=min(avg, (1 << 32) - 1))
    if isinstance(dest, (str, os.PathLike)):
        with open(dest, "wb") as f:
            f.write(data)
    else:
        dest.write(data)
    return len(data)


def save(dest, pcm, sample_rate, sample_size=16, frame_length=4096, device=0):
    """Encode pcm [C, T] (planar, torch int32 -- the canonical sample -- or float32 -- sample * 2^-(bits-1), what `load`
    returns) on the GPU to ALAC and write it as an M4A file to `dest` (a path or a writable binary file object).  Returns the
    file's size in bytes.  int32 samples outside the sample range are clamped to it.  float32 samples are multiplied by
    2^(sample_size-1) in float32, clamped to the sample range (so +-1.0 and beyond, and +-inf, give the extremes), then
    rounded to the nearest integer, half to even; NaN gives the smallest sample.  ValueError (before any device work) for a channel count other than 1 / 2, a sample size other than
    16 / 24, a frame_length outside 1 .. 16384, a tensor that is not on the GPU, an empty input, or a length whose file could
    outgrow the 32-bit chunk offsets."""
    F, C_, T = _check_save_args(pcm, False, sample_size, frame_length, sample_rate)
    _check_stco(T, C_, sample_size, int(frame_length))
    if pcm.device.type != "cuda":
        raise ValueError("pcm must be on the GPU")
    packets, durations = _encode_tensor(pcm.unsqueeze(0), [T], sample_size, int(frame_length), device)
    return _write_file(dest, packets[0], durations[0], int(frame_length), sample_size, C_, int(sample_rate))


def _check_batch_args(pcm, lengths, sample_rate, sample_size, frame_length, dests=None):
    """The host-side checks of save_batch and Corpus.from_pcm for one batch, before any device work; returns (F, C, T, the
    lengths as a list of ints)."""
    F, C_, T = _check_save_args(pcm, True, sample_size, frame_length, sample_rate)
    lengths = [int(x) for x in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if dests is not None and len(dests) != F or len(lengths) != F:
        raise ValueError(f"{F} files in pcm, " + (f"{len(dests)} destinations and " if dests is not None else "") + f"{len(lengths)} lengths")
    for L in lengths:
        if not 1 <= L <= T:
            raise ValueError(f"length {L} outside 1 .. {T}")
        _check_stco(L, C_, sample_size, int(frame_length))
    if pcm.device.type != "cuda":
        raise ValueError("pcm must be on the GPU")
    return F, C_, T, lengths


def save_batch(dests, pcm, lengths, sample_rate, sample_size=16, frame_length=4096, device=0):
    """`save` for F files in ONE launch: file f is frames 0 .. lengths[f] of pcm[f] ([F, C, Tmax], as `load_batch` returns
    it); dests[f] a path or a writable binary file object.  Returns the file sizes."""
    F, C_, T, lengths = _check_batch_args(pcm, lengths, sample_rate, sample_size, frame_length, dests)
    packets, durations = _encode_tensor(pcm, lengths, sample_size, int(frame_length), device)
    return [_write_file(d, packets[f], durations[f], int(frame_length), sample_size, C_, int(sample_rate))
            for f, d in enumerate(dests)]


class AlacFile:
    """Mirror of the reference's `internal class AlacFile` surface for the path (AlacFile.cs:14-20,
    :63, :428) on the GPU library: same names, argument meaning and error behaviour; plus DecodeBatch."""

    def __init__(self, samplesize, numchannels, device=0):
        self._samplesize = samplesize
        self._numchannels = numchannels
        self._device = device
        self._ctx = None
        self._cfg = None

    def SetInfo(self, inputbuffer):
        self._cfg = cfg_from_codec_data(inputbuffer, self._samplesize, self._numchannels)
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = AlacGpuContext(self._cfg, self._device)

    def DecodeFrame(self, inbuffer, outbuffer):
        """int DecodeFrame(byte[] inbuffer, int[] outbuffer): fills outbuffer in the reference's layout,
        returns the byte count (AlacFile.cs:718)."""
        if self._ctx is None:
            raise Exception("SetInfo must be called first")
        ref, out_bytes, st = self._ctx.decode_frame(0, inbuffer)
        if st == ST_UNSUPPORTED_ELEMENT:
            return out_bytes  # reference decodes nothing and still returns outputsize (:437,:577,:718)
        if (st == ST_UNSUPPORTED_SAMPLE_SIZE and len(inbuffer) and (int(inbuffer[0]) >> 5) == 1
                and int(self._cfg[0]["sample_size"]) not in (20, 32)):
            return out_bytes  # a two-channel element of any other sample size: nothing is written, no exception (:701-716)
        if st == ST_UNSUPPORTED_PREDTYPE and len(inbuffer) and (int(inbuffer[0]) >> 5) == 0:
            # one-channel element with a prediction type other than 0: the reference skips the predictor without a word and
            # hands out _outputsamplesBufferA (AlacFile.cs:484-496) -- which, once a compressed frame has been decoded, IS
            # the residual buffer (:486): the un-predicted residuals, which is what the library returns with status 3.
            # (A decoder that has never decoded a compressed frame would show zeros there: not reproduced)
            n = min(len(outbuffer), len(ref))
            outbuffer[:n] = ref[:n]
            return out_bytes
        _raise_reference_exception(st, int(self._cfg[0]["sample_size"]))
        n = min(len(outbuffer), len(ref))
        outbuffer[:n] = ref[:n]
        return out_bytes

    def DecodeBatch(self, blob, offsets, sizes, slot_ints=None):
        """Batch-submit entry point (north_star: "AlacContext gains a batch-submit entry point")."""
        if self._ctx is None:
            raise Exception("SetInfo must be called first")
        return self._ctx.decode_batch(blob, offsets, sizes, None, slot_ints)

    def Dispose(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


# ---- a corpus resident in HBM and its random crops (alacgpu_plan_crops_device) -----------------------------------------------------
from .corpus import (Corpus, compact_plan_host, corpus_plan_host, corpus_tables, entries_per_crop,  # noqa: E402  (it imports the names above)
                     stage_bytes_per_crop, stage_plan_host, tier_split)
# ---- crops and tensors at another sample rate (alacgpu_resample_device) ---------------------------------------------------------------
from .resample import resample, resample_host, resample_table, source_window  # noqa: E402
# ---- log-mel features of crops and tensors (alacgpu_logmel_device) -----------------------------------------------------------------
from .features import LogMel, log_mel, logmel_host, logmel_host_f32, mel_filterbank  # noqa: E402
# ---- Kaldi filterbank features of crops and tensors (alacgpu_fbank_device) ----------------------------------------------------------
from .fbank import KaldiFbank, fbank, fbank_host, fbank_host_f32, fbank_lengths, kaldi_mel_banks, kaldi_window  # noqa: E402
# ---- Kaldi MFCC features of crops and tensors (alacgpu_mfcc_device) and delta features behind any features (alacgpu_deltas_device) --
from .mfcc import KaldiMfcc, kaldi_dct, kaldi_lifter, mfcc, mfcc_host, mfcc_host_f32  # noqa: E402
from .deltas import Deltas, add_deltas, delta_scales, deltas_host, deltas_host_f32  # noqa: E402

# ---- normalised crops and features (alacgpu_normalize_meanvar_device, alacgpu_normalize_top_device) ------------------------------
from .normalize import MeanVar, TopDb, normalize, normalize_host, normalize_host_f32  # noqa: E402

# ---- Kaldi's sliding-window CMVN, a third kind of normalize's `how` (alacgpu_normalize_sliding_device), and the energy VAD with
# ---- the selection of the voiced frames (alacgpu_vad_energy_device, alacgpu_select_frames_device) ---------------------------------
from .sliding import SlidingMeanVar, sliding_host, sliding_host_f32, sliding_windows  # noqa: E402
# ---- per-channel energy normalisation, a fourth kind of normalize's `how` (alacgpu_pcen_device) --------------------------------------
from .pcen import Pcen, pcen, pcen_host, pcen_host_f32, pcen_smoother_host, pcen_smoother_host_f32  # noqa: E402
from .vad import EnergyVad, select_frames, select_host, vad_energy, vad_host, vad_host_f32  # noqa: E402
# ---- noise at a target signal-to-noise ratio into crops and tensors (alacgpu_mix_device) ----------------------------------------
from .mix import AddNoise, mix, mix_host, mix_host_f32  # noqa: E402
# ---- biquad filters and a gain on crops and tensors (alacgpu_biquad_device) ----------------------------------------------------------
from .biquad import (Effects, RandomBiquad, allpass, bandpass, bandreject, biquad, biquad_host, biquad_host_twin, highpass,  # noqa: E402
                     highshelf, lowpass, lowshelf, peaking)
# ---- peak, RMS and loudness levelling of crops and tensors (alacgpu_level_device) --------------------------------------------------
from .level import Level, kweight, level, level_host, level_host_twin, loudness, loudness_host  # noqa: E402
# ---- constant-Q features of crops and tensors (alacgpu_cqt_device) --------------------------------------------------------------------
from .cqt import ConstantQ, cqt, cqt_frequencies, cqt_host, cqt_host_f32, cqt_lengths, cqt_work  # noqa: E402
# ---- linear, complex and banded spectrograms of crops and tensors (alacgpu_stft_device) -----------------------------------------------
from .stft import Spectrogram, as_complex, spectrogram, spectrogram_host, spectrogram_host_f32  # noqa: E402
# ---- F0 contours of crops and tensors: the YIN estimator (alacgpu_yin_device) ----------------------------------------------------------
from .yin import Yin, hz_to_cents, yin, yin_host, yin_host_f32  # noqa: E402

# ---- smoothed F0 tracks: probabilistic YIN with a Viterbi decode (alacgpu_pyin_device) ---------------------------------------------------
from .pyin import PYin, pyin, pyin_decode, pyin_host, pyin_host_f32, pyin_observation  # noqa: E402

# ---- Kaldi's pitch features: NCCF on a lag grid, a dense Viterbi decode, the post-processing (alacgpu_kaldi_pitch_device) -----------------
from .kaldi_pitch import (KaldiPitch, kaldi_pitch, kaldi_pitch_decode, kaldi_pitch_host, kaldi_pitch_host_f32, kaldi_pitch_nccf,  # noqa: E402
                          kaldi_pitch_process)

# ---- pitch shift and time stretch of crops and tensors (alacgpu_time_stretch_device) ------------------------------------------------
from .pitch import (PitchShift, pitch_shift, pitch_shift_host, pitch_shift_host_f32, semitone_ratio, time_stretch,  # noqa: E402
                    time_stretch_host, time_stretch_host_f32)
# ---- room reverberation into crops and tensors (alacgpu_reverb_device) ------------------------------------------------------------
from .reverb import Reverb, reverb, reverb_host, reverb_host_f32  # noqa: E402

# ---- simulated room responses behind Reverb (alacgpu_rir_shoebox_device) -----------------------------------------------------------
from .rir import ShoeboxRooms, image_counts, rir_host, rir_host_f32, simulate_rir  # noqa: E402
# ---- SpecAugment on the features: time warp, frequency and time masks (alacgpu_specaugment_device) -------------------------------
from .augment import SpecAugment, spec_augment, specaugment_host, specaugment_host_f32  # noqa: E402
from .speed import SpeedPerturb, speed_host, speed_host_f32, speed_perturb  # noqa: E402
