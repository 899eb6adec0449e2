// alacgpu_stages.hip -- C ABI of include/alacgpu.h, the stages around the decode: the crop planner, the scan with the packet
// compaction and staging, the resamplers, log-mel, Kaldi fbank and MFCC, the delta features, the phase vocoder, the reverberation, the simulated room responses, the noise mix, the levelling, the biquad cascade, the YIN pitch estimator, probabilistic YIN with its Viterbi decode, the constant-Q transform, the STFT, the normalisations, the per-channel energy normalisation, the energy VAD with the selection of the voiced frames, SpecAugment and the encoder.  Of the ctx they use the device, the cfgs, last_error and
// their own scratch; the decode path is alacgpu_api.hip.  No CPU fallback here either: every stage is its kernels.
#include <algorithm>
#include <cmath>
#include <vector>

#include "alac_corpus.h"
#include "alac_resample.h"
#include "alac_features.h"
#include "alac_fbank.h"
#include "alac_mfcc.h"
#include "alac_deltas.h"
#include "alac_normalize.h"
#include "alac_sliding.h"
#include "alac_pcen.h"
#include "alac_vad.h"
#include "alac_augment.h"
#include "alac_mix.h"
#include "alac_biquad.h"
#include "alac_yin.h"
#include "alac_pyin.h"
#include "alac_kaldi_pitch.h"
#include "alac_cqt.h"
#include "alac_stft.h"
#include "alac_level.h"
#include "alac_reverb.h"
#include "alac_rir.h"
#include "alac_stretch.h"
#include "alac_encode.h"
#include "alacgpu_ctx.h"

namespace {

// Both planner entry points; each: every crop has a window length of its own, d_crop_frames[n_crops]
int plan_crops(alacgpu_ctx* ctx, const void* d_pkt_offset, const void* d_pkt_size, const void* d_pkt_end,
               const void* d_file_first, const void* d_file_cfg, uint32_t n_files, const void* d_crop_file,
               const void* d_crop_offset, bool each, const void* d_crop_frames, uint32_t n_crops, uint32_t crop_frames,
               uint32_t entries_per_crop, uint64_t dst_stride, void* d_offsets, void* d_sizes, void* d_cfg_idx,
               void* d_dst_first, void* d_dst_frames, void* d_src_skip, void* d_lengths, void* hip_stream) {
    if (!ctx) return ALACGPU_ERR_BAD_ARG;
    if (n_crops == 0) return ALACGPU_OK;
    if (entries_per_crop == 0 || (uint64_t)n_crops * entries_per_crop > 0xFFFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (!args_ok({{d_pkt_offset, 8}, {d_pkt_size, 4}, {d_pkt_end, 8}, {d_file_first, 4}, {d_file_cfg, 2}, {d_crop_file, 4},
                  {d_crop_offset, 8}, {d_crop_frames, 4, each}, {d_offsets, 8}, {d_sizes, 4}, {d_cfg_idx, 2}, {d_dst_first, 8},
                  {d_dst_frames, 4}, {d_src_skip, 4}, {d_lengths, 8}}))
        return ALACGPU_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_plan_params p;
    p.pkt_offset = (const uint64_t*)d_pkt_offset;
    p.pkt_size = (const uint32_t*)d_pkt_size;
    p.pkt_end = (const uint64_t*)d_pkt_end;
    p.file_first = (const uint32_t*)d_file_first;
    p.file_cfg = (const uint16_t*)d_file_cfg;
    p.n_files = n_files;
    p.crop_file = (const uint32_t*)d_crop_file;
    p.crop_offset = (const uint64_t*)d_crop_offset;
    p.n_crops = n_crops;
    p.crop_frames = crop_frames;
    p.crop_frames_each = each ? (const uint32_t*)d_crop_frames : nullptr;
    p.entries_per_crop = entries_per_crop;
    p.dst_stride = dst_stride;
    p.offsets = (uint64_t*)d_offsets;
    p.sizes = (uint32_t*)d_sizes;
    p.cfg_idx = (uint16_t*)d_cfg_idx;
    p.dst_first = (uint64_t*)d_dst_first;
    p.dst_frames = (uint32_t*)d_dst_frames;
    p.src_skip = (uint32_t*)d_src_skip;
    p.lengths = (int64_t*)d_lengths;
    constexpr uint32_t per_wg = ALAC_PLAN_THREADS / 64;   // one wave per crop
    void* kargs[] = {&p};
    const void* const kernel = each ? (const void*)alac_plan_crops_frames_kernel : (const void*)alac_plan_crops_kernel;
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((n_crops + per_wg - 1u) / per_wg), dim3(ALAC_PLAN_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

// The exclusive scan both alacgpu_compact_packets_device and alacgpu_stage_packets_device begin with: s0 holds the sizes, how
// they count, `add`, `out` and `total`; the two kernels are the level-0 pair that counts that way.  The levels: the sizes, the
// sums of their tiles, the sums of those sums' tiles (at most 1024 for 2^32 - 1 packets), in the ctx's scratch (none for one tile).
int scan_sizes(alacgpu_ctx* ctx, alac_scan_params<uint32_t> s0, const void* sums_kernel, const void* tiles_kernel, hipStream_t stream) {
    const uint64_t t1 = (s0.n + ALAC_SCAN_TILE - 1u) / ALAC_SCAN_TILE;
    const uint64_t t2 = (t1 + ALAC_SCAN_TILE - 1u) / ALAC_SCAN_TILE;
    const size_t need = t1 > 1 ? sizeof(uint64_t) * (size_t)(t1 + t2) : 0;
    int rc = ctx->scan.acquire(ctx, stream, need, align_up(need + need / 4, 4096));
    if (rc) return rc;
    uint64_t* const l1 = t1 > 1 ? (uint64_t*)ctx->scan.buf[0] : nullptr;   // (one tile: the call owns none of the buffer, and gets none)
    uint64_t* const l2 = l1 ? l1 + t1 : nullptr;
    s0.sums = l1;
    s0.tile_base = l1;
    const dim3 block(ALAC_SCAN_THREADS);
    if (t1 > 1) {
        alac_scan_params<uint64_t> s1 = {};
        s1.in = l1;
        s1.n = t1;
        s1.slot_bytes = 0;
        s1.sums = l2;
        s1.tile_base = t2 > 1 ? l2 : nullptr;
        s1.add = 0;
        s1.out = l1;
        s1.total = nullptr;
        void* a0[] = {&s0};
        void* a1[] = {&s1};
        HIP_TRY(ctx, hipLaunchKernel(sums_kernel, dim3((uint32_t)t1), block, a0, 0, stream));
        if (t2 > 1) {
            alac_scan_params<uint64_t> s2 = s1;          // t2 <= 1024: one tile
            s2.in = l2;
            s2.n = t2;
            s2.sums = nullptr;
            s2.tile_base = nullptr;
            s2.out = l2;
            void* a2[] = {&s2};
            HIP_TRY(ctx, hipLaunchKernel((const void*)alac_scan_sums_u64_kernel, dim3((uint32_t)t2), block, a1, 0, stream));
            HIP_TRY(ctx, hipLaunchKernel((const void*)alac_scan_tiles_u64_kernel, dim3(1), block, a2, 0, stream));
        }
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_scan_tiles_u64_kernel, dim3((uint32_t)t2), block, a1, 0, stream));
    }
    void* a0[] = {&s0};
    HIP_TRY(ctx, hipLaunchKernel(tiles_kernel, dim3((uint32_t)t1), block, a0, 0, stream));
    return ALACGPU_OK;
}

// What alacgpu_compact_packets_device and alacgpu_stage_packets_device begin and end with.  scan_begin: the ctx and d_total
// checked and the device made current; without packets (done) d_total[0] = 0 is the whole call.  scan_end releases the scratch.
int scan_begin(alacgpu_ctx* ctx, void* d_total, uint32_t n_packets, hipStream_t stream, bool& done) {
    done = n_packets == 0;
    if (!ctx || !args_ok({{d_total, 8}})) return ALACGPU_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (done) HIP_TRY(ctx, hipMemsetAsync(d_total, 0, sizeof(uint64_t), stream));
    return ALACGPU_OK;
}

int scan_end(alacgpu_ctx* ctx, hipStream_t stream) {
    HIP_TRY(ctx, hipGetLastError());
    return ctx->scan.release(ctx, stream);
}

// The tile of a resample launch: as many output frames as leave a CU room for two workgroups, down to 256; fewer only where the
// span of 256 does not fit the CU at all (a / b in the hundreds) -- one frame's span, 2 width + 2, always fits next to the table.
// lds_bytes(tile): the dynamic LDS a workgroup needs for that tile.
template <class F>
uint32_t resample_tile(const F& lds_bytes) {
    uint32_t tile = ALAC_RESAMPLE_MAX_TILE;
    while (tile > 256u && lds_bytes(tile) > ALAC_RESAMPLE_LDS_PREFERRED) tile /= 2u;
    while (tile > 1u && lds_bytes(tile) > ALAC_RESAMPLE_LDS_MAX) tile /= 2u;
    return tile;
}

// The grid: a workgroup takes up to eight consecutive tiles with one load of the table, while a thousand workgroups remain.
// false: 2^31 tiles of output or more.
bool resample_grid(uint64_t out_frames, uint32_t tile, uint64_t planes, uint32_t& per_wg, uint32_t& blocks) {
    const uint64_t tiles = (out_frames + tile - 1u) / tile;
    if (tiles > 0xFFFFFFFFull || tiles * planes > 0x7FFFFFFFull) return false;
    const uint64_t n = std::min<uint64_t>(std::max<uint64_t>(tiles * planes / 1024u, 1u), std::min<uint64_t>(tiles, ALAC_RESAMPLE_MAX_TILES_PER_WG));
    per_wg = (uint32_t)n;
    blocks = (uint32_t)((tiles + n - 1u) / n * planes);
    return true;
}

// What the three resample entries share, behind the checks of their own tables or ratios: the pointers they have in common, the
// launch's tile, grid and LDS from lds_bytes(tile), the alac_resample_io their parameter structs contain -- own(p, tile, lds) sets
// the fields that differ -- and the launch.
template <class P, class F, class G>
int resample(alacgpu_ctx* ctx, const void* kernel, const F& lds_bytes, const G& own, const void* d_src, uint32_t rows, uint32_t channels,
             uint64_t src_stride, const void* d_src_origin, const void* d_src_valid, const void* d_out_first, uint64_t out_frames,
             int mono, void* d_out, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_src_origin, 8}, {d_src_valid, 8}, {d_out_first, 8}, {d_out, 4}}) || channels < 1 || channels > 2)
        return ALACGPU_ERR_BAD_ARG;
    if (rows == 0 || out_frames == 0) return ALACGPU_OK;
    const uint32_t tile = resample_tile(lds_bytes);
    const size_t lds = lds_bytes(tile);
    uint32_t per_wg, blocks;
    if (!resample_grid(out_frames, tile, (uint64_t)rows * (mono ? 1u : channels), per_wg, blocks)) return ALACGPU_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (lds > ALAC_RESAMPLE_LDS_PREFERRED) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    P p;
    p.io = {(const float*)d_src, src_stride, (const int64_t*)d_src_origin, (const int64_t*)d_src_valid, (const int64_t*)d_out_first,
            (float*)d_out, out_frames, channels, mono ? 1u : 0u, tile, per_wg};
    own(p, tile, lds);
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3(blocks), dim3(ALAC_RESAMPLE_THREADS), kargs, lds, (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

// What the two normalisations share in front of their own limits: the ctx and the arrays, the shape of the lines, and d_src
// and d_out either the same array or apart.  lines: rows * lines_per_row
bool normalize_args_ok(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row, uint64_t line_stride,
                       uint64_t line_len, uint64_t& lines) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}}) || lines_per_row == 0 || line_len == 0 || line_len > line_stride) return false;
    lines = (uint64_t)rows * lines_per_row;
    if (line_stride > (1ull << 60) / sizeof(float) / std::max<uint64_t>(lines, 1u)) return false;      // (the extent fits 60 bits)
    const uint64_t extent = lines ? sizeof(float) * ((lines - 1u) * line_stride + line_len) : 0u;
    const uintptr_t a = (uintptr_t)d_src, b = (uintptr_t)d_out;
    return a == b || a + extent <= b || b + extent <= a;
}

// The bytes from the first element of float32 [planes, stride], of which the first `len` of a plane are data, to behind its
// last; false: 2^60 bytes or more
bool planes_extent(uint64_t planes, uint64_t stride, uint64_t len, uint64_t& extent) {
    if (stride > (1ull << 60) / sizeof(float) / std::max<uint64_t>(planes, 1u)) return false;
    extent = planes ? sizeof(float) * ((planes - 1u) * stride + len) : 0u;
    return true;
}

bool apart(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    return (uintptr_t)a + a_bytes <= (uintptr_t)b || (uintptr_t)b + b_bytes <= (uintptr_t)a;
}

// What alacgpu_logmel_device, alacgpu_fbank_device and alacgpu_mfcc_device do behind their own argument checks: the grid of tiles, the LDS layout
// (with `extra` floats of the kernel's own), the shared fields of p and the launch of `kernel`, whose argument p is
template <typename Params>
int launch_stft_mel(alacgpu_ctx* ctx, const void* kernel, Params& p, uint32_t extra, const void* d_src, uint32_t rows,
                           uint32_t channels, uint64_t src_stride, uint64_t frames, uint32_t taps, uint32_t n_fft, uint32_t hop,
                           uint32_t n_mels, const void* d_window, const void* d_basis, const void* d_fb, void* d_out,
                           uint64_t out_frames, void* hip_stream) {
    const uint32_t tile = alac_features_tile(taps, hop);
    const uint64_t tiles = (out_frames + tile - 1u) / tile;
    if (tiles > 0x7FFFFFFFull || tiles * channels > 0x7FFFFFFFull || tiles * channels * rows > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    const size_t lds = alac_features_lds_layout(taps, n_fft, hop, n_mels, extra).bytes();
    if (lds > ALAC_FEATURES_LDS_MAX) return ALACGPU_ERR_BAD_ARG;    // (the callers' limits keep every layout below it)
    if (rows == 0 || out_frames == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (lds > ALAC_FEATURES_LDS_DEFAULT) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    p.src = (const float*)d_src;
    p.src_stride = src_stride;
    p.frames = frames;
    p.out = (float*)d_out;
    p.out_frames = out_frames;
    p.window = (const float*)d_window;
    p.basis = (const float*)d_basis;
    p.fb = (const float*)d_fb;
    p.taps = taps;
    p.n_fft = n_fft;
    p.hop = hop;
    p.n_mels = n_mels;
    p.tile = tile;
    p.tiles = (uint32_t)tiles;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((uint32_t)(tiles * channels * rows)), dim3(ALAC_FEATURES_THREADS), kargs, lds,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

}  // namespace

extern "C" {

int alacgpu_plan_crops_device(alacgpu_ctx* ctx, const void* d_pkt_offset, const void* d_pkt_size, const void* d_pkt_end,
                              const void* d_file_first, const void* d_file_cfg, uint32_t n_files, const void* d_crop_file,
                              const void* d_crop_offset, uint32_t n_crops, uint32_t crop_frames, uint32_t entries_per_crop,
                              uint64_t dst_stride, void* d_offsets, void* d_sizes, void* d_cfg_idx, void* d_dst_first,
                              void* d_dst_frames, void* d_src_skip, void* d_lengths, void* hip_stream) {
    return plan_crops(ctx, d_pkt_offset, d_pkt_size, d_pkt_end, d_file_first, d_file_cfg, n_files, d_crop_file, d_crop_offset, false,
                      nullptr, n_crops, crop_frames, entries_per_crop, dst_stride, d_offsets, d_sizes, d_cfg_idx, d_dst_first,
                      d_dst_frames, d_src_skip, d_lengths, hip_stream);
}

int alacgpu_plan_crops_frames_device(alacgpu_ctx* ctx, const void* d_pkt_offset, const void* d_pkt_size, const void* d_pkt_end,
                                     const void* d_file_first, const void* d_file_cfg, uint32_t n_files, const void* d_crop_file,
                                     const void* d_crop_offset, const void* d_crop_frames, uint32_t n_crops, uint32_t crop_frames,
                                     uint32_t entries_per_crop, uint64_t dst_stride, void* d_offsets, void* d_sizes,
                                     void* d_cfg_idx, void* d_dst_first, void* d_dst_frames, void* d_src_skip, void* d_lengths,
                                     void* hip_stream) {
    return plan_crops(ctx, d_pkt_offset, d_pkt_size, d_pkt_end, d_file_first, d_file_cfg, n_files, d_crop_file, d_crop_offset, true,
                      d_crop_frames, n_crops, crop_frames, entries_per_crop, dst_stride, d_offsets, d_sizes, d_cfg_idx, d_dst_first,
                      d_dst_frames, d_src_skip, d_lengths, hip_stream);
}

int alacgpu_compact_packets_device(alacgpu_ctx* ctx, const void* d_packets, uint64_t slot_bytes, const void* d_sizes,
                                   uint32_t n_packets, void* d_blob, uint64_t base, uint64_t blob_capacity,
                                   void* d_pkt_offset, void* d_total, void* hip_stream) {
    if (slot_bytes == 0 || (slot_bytes & 15u) != 0) return ALACGPU_ERR_BAD_ARG;
    hipStream_t stream = (hipStream_t)hip_stream;
    bool done;
    int rc = scan_begin(ctx, d_total, n_packets, stream, done);
    if (rc || done) return rc;
    if (!args_ok({{d_packets, 16}, {d_sizes, 4}, {d_blob, 1}, {d_pkt_offset, 8}})) return ALACGPU_ERR_BAD_ARG;
    alac_scan_params<uint32_t> s0 = {};
    s0.in = (const uint32_t*)d_sizes;
    s0.n = n_packets;
    s0.slot_bytes = slot_bytes;
    s0.add = base;
    s0.out = (uint64_t*)d_pkt_offset;
    s0.total = (uint64_t*)d_total;
    scratch_hold hold{ctx->scan, stream};
    if ((rc = scan_sizes(ctx, s0, (const void*)alac_scan_sums_u32_kernel, (const void*)alac_scan_tiles_u32_kernel, stream))) return rc;
    // the copy: tiles of the destination, as many as the packets can fill at most (the true end is d_total's, on the device)
    const uint64_t most = slot_bytes > UINT64_MAX / n_packets ? UINT64_MAX : slot_bytes * n_packets;
    const uint64_t room = blob_capacity > base ? blob_capacity - base : 0;
    const uint64_t bound = std::min(most, room);
    if (bound) {
        alac_copy_params c;
        c.packets = (const uint8_t*)d_packets;
        c.slot_bytes = slot_bytes;
        c.sizes = (const uint32_t*)d_sizes;
        c.pkt_offset = (const uint64_t*)d_pkt_offset;
        c.total = (const uint64_t*)d_total;
        c.n_packets = n_packets;
        c.blob = (uint8_t*)d_blob;
        c.base = base;
        c.capacity = blob_capacity;
        const uint64_t tiles = bound / ALAC_COPY_TILE + 2u;   // (a tile more for the bytes in front of the first aligned chunk)
        void* ac[] = {&c};
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_compact_copy_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, 1u << 16)),
                                     dim3(ALAC_COPY_THREADS), ac, 0, stream));
    }
    return scan_end(ctx, stream);
}

int alacgpu_stage_packets_device(alacgpu_ctx* ctx, const void* d_blob_lo, uint64_t lo_bytes, const void* blob_hi, uint64_t hi_bytes,
                                 const void* d_src_offset, const void* d_sizes, uint32_t n_packets, void* d_stage,
                                 uint64_t stage_capacity, void* d_stage_offset, void* d_total, void* hip_stream) {
    if (!args_ok({{d_blob_lo, 16, lo_bytes != 0}, {blob_hi, 16, hi_bytes != 0}})) return ALACGPU_ERR_BAD_ARG;
    hipStream_t stream = (hipStream_t)hip_stream;
    bool done;
    int rc = scan_begin(ctx, d_total, n_packets, stream, done);
    if (rc || done) return rc;
    if (!args_ok({{d_src_offset, 8}, {d_sizes, 4}, {d_stage, 16}, {d_stage_offset, 8}}) || lo_bytes > UINT64_MAX - hi_bytes)
        return ALACGPU_ERR_BAD_ARG;
    // the second part as the kernels address it: device memory as it is, page-locked host memory by its device view
    const void* hi_view = nullptr;
    if (hi_bytes) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, blob_hi) != hipSuccess) { (void)hipGetLastError(); return ALACGPU_ERR_BAD_ARG; }
        hi_view = a.type == hipMemoryTypeDevice ? blob_hi : device_view_of_pinned(blob_hi, (size_t)hi_bytes);
        if (!hi_view) return ALACGPU_ERR_BAD_ARG;
    }
    alac_scan_params<uint32_t> s0 = {};
    s0.in = (const uint32_t*)d_sizes;
    s0.n = n_packets;
    s0.src_offset = (const uint64_t*)d_src_offset;
    s0.lo_bytes = lo_bytes;
    s0.hi_bytes = hi_bytes;
    s0.out = (uint64_t*)d_stage_offset;
    s0.total = (uint64_t*)d_total;
    scratch_hold hold{ctx->scan, stream};
    if ((rc = scan_sizes(ctx, s0, (const void*)alac_scan_sums_stage_kernel, (const void*)alac_scan_tiles_stage_kernel, stream))) return rc;
    // the copy: tiles of the staging blob, as many as its capacity holds (the true end is d_total's, on the device)
    if (stage_capacity >= 16u) {
        alac_stage_params c;
        c.lo = (const uint8_t*)d_blob_lo;
        c.hi = (const uint8_t*)hi_view;
        c.lo_bytes = lo_bytes;
        c.hi_bytes = hi_bytes;
        c.src_offset = (const uint64_t*)d_src_offset;
        c.sizes = (const uint32_t*)d_sizes;
        c.stage_offset = (const uint64_t*)d_stage_offset;
        c.total = (const uint64_t*)d_total;
        c.n_packets = n_packets;
        c.stage = (uint8_t*)d_stage;
        c.capacity = stage_capacity;
        const uint64_t tiles = stage_capacity / ALAC_STAGE_TILE + 1u;
        void* ac[] = {&c};
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_stage_copy_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, 1u << 16)),
                                     dim3(ALAC_STAGE_THREADS), ac, 0, stream));
    }
    return scan_end(ctx, stream);
}

int alacgpu_resample_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                            const void* d_src_origin, const void* d_src_valid, const void* d_out_first, uint64_t out_frames,
                            uint32_t a, uint32_t b, uint32_t width, const void* d_d0, const void* d_weights, int mono, void* d_out,
                            void* hip_stream) {
    const uint64_t table = (uint64_t)b * (2u * (uint64_t)width + 1u);
    if (!args_ok({{d_d0, 4}, {d_weights, 4}}) || a == 0 || b == 0 || width == 0 || table > ALAC_RESAMPLE_MAX_TABLE) return ALACGPU_ERR_BAD_ARG;
    const auto lds_bytes = [&](uint64_t tile) { return sizeof(float) * (size_t)(((table + 3u) & ~3ull) + alac_resample_span(tile, a, b, width)); };
    const auto own = [&](alac_resample_params& p, uint32_t tile, size_t lds) {
        p.d0 = (const int32_t*)d_d0;
        p.weights = (const float*)d_weights;
        p.a = a;
        p.b = b;
        p.width = width;
        p.span = (uint32_t)alac_resample_span(tile, a, b, width);
    };
    return resample<alac_resample_params>(ctx, (const void*)alac_resample_kernel, lds_bytes, own, d_src, rows, channels, src_stride,
                                          d_src_origin, d_src_valid, d_out_first, out_frames, mono, d_out, hip_stream);
}

static_assert(sizeof(alacgpu_resample_table) == sizeof(alac_resample_table) && offsetof(alacgpu_resample_table, weights_first) ==
              offsetof(alac_resample_table, weights_first), "the kernel reads the header's table descriptors as they are");

int alacgpu_resample_rows_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                                 const void* d_src_origin, const void* d_src_valid, const void* d_out_first, uint64_t out_frames,
                                 const alacgpu_resample_table* tables, const void* d_tables, uint32_t n_tables, const void* d_d0,
                                 const void* d_weights, const void* d_row_table, int mono, void* d_out, void* hip_stream) {
    if (!args_ok({{tables, 4}, {d_tables, 4}, {d_d0, 4}, {d_weights, 4}, {d_row_table, 4}}) || n_tables == 0) return ALACGPU_ERR_BAD_ARG;
    for (uint32_t t = 0; t < n_tables; t++) {
        const alacgpu_resample_table& d = tables[t];
        if (d.a == 0 || d.b == 0 || d.width == 0 || (uint64_t)d.b * (2u * (uint64_t)d.width + 1u) > ALAC_RESAMPLE_MAX_TABLE)
            return ALACGPU_ERR_BAD_ARG;
    }
    // one tile for the launch, and the LDS of the table that needs the most for it; a workgroup uses its own table's span
    const auto lds_bytes = [&](uint64_t tile) {
        uint64_t most = 0;
        for (uint32_t t = 0; t < n_tables; t++) {
            const alacgpu_resample_table& d = tables[t];
            const uint64_t table = (uint64_t)d.b * (2u * (uint64_t)d.width + 1u);
            most = std::max<uint64_t>(most, ((table + 3u) & ~3ull) + alac_resample_span(tile, d.a, d.b, d.width));
        }
        return sizeof(float) * (size_t)most;
    };
    const auto own = [&](alac_resample_rows_params& p, uint32_t tile, size_t lds) {
        p.tables = (const alac_resample_table*)d_tables;
        p.d0 = (const int32_t*)d_d0;
        p.weights = (const float*)d_weights;
        p.row_table = (const uint32_t*)d_row_table;
        p.n_tables = n_tables;
        p.lds_floats = (uint32_t)(lds / sizeof(float));
    };
    return resample<alac_resample_rows_params>(ctx, (const void*)alac_resample_rows_kernel, lds_bytes, own, d_src, rows, channels,
                                               src_stride, d_src_origin, d_src_valid, d_out_first, out_frames, mono, d_out, hip_stream);
}

static_assert(sizeof(alacgpu_resample_ratio) == sizeof(alac_resample_ratio) && offsetof(alacgpu_resample_ratio, width) ==
              offsetof(alac_resample_ratio, width), "the kernel reads the header's ratios as they are");

int alacgpu_resample_ratio_rows_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                                       const void* d_src_origin, const void* d_src_valid, const void* d_out_first, uint64_t out_frames,
                                       const alacgpu_resample_ratio* ratios, const void* d_ratios, uint32_t n_ratios,
                                       const void* d_row_ratio, int mono, void* d_out, void* hip_stream) {
    if (!args_ok({{ratios, 4}, {d_ratios, 4}, {d_row_ratio, 4}}) || n_ratios == 0) return ALACGPU_ERR_BAD_ARG;
    bool any = false;
    for (uint32_t t = 0; t < n_ratios; t++) {
        const alacgpu_resample_ratio& d = ratios[t];
        if (d.b == 0 || d.a >= (1u << 31) || d.b >= (1u << 31)) return ALACGPU_ERR_BAD_ARG;
        // a ratio that is used: a frame's span, 2 width + 2, has to fit the LDS of a CU (a / b up to about 3378)
        if (d.a != 0 && (d.width == 0 || d.width > ALAC_RESAMPLE_RATIO_MAX_WIDTH)) return ALACGPU_ERR_BAD_ARG;
        any = any || d.a != 0;
    }
    // one tile for the launch, and the LDS of the ratio whose span of it is the longest; a workgroup uses its own ratio's span
    const auto lds_bytes = [&](uint64_t tile) {
        uint64_t most = 0;
        for (uint32_t t = 0; t < n_ratios; t++)
            if (ratios[t].a != 0) most = std::max<uint64_t>(most, alac_resample_span(tile, ratios[t].a, ratios[t].b, ratios[t].width));
        return sizeof(float) * (size_t)most;
    };
    const auto own = [&](alac_resample_ratio_params& p, uint32_t tile, size_t lds) {
        p.ratios = (const alac_resample_ratio*)d_ratios;
        p.row_ratio = (const uint32_t*)d_row_ratio;
        p.n_ratios = n_ratios;
        p.lds_floats = (uint32_t)(lds / sizeof(float));
    };
    // (every ratio with a == 0: the shared checks still run, with no output frames nothing is launched)
    return resample<alac_resample_ratio_params>(ctx, (const void*)alac_resample_ratio_rows_kernel, lds_bytes, own, d_src, rows, channels,
                                                src_stride, d_src_origin, d_src_valid, d_out_first, any ? out_frames : 0u, mono, d_out,
                                                hip_stream);
}

int alacgpu_logmel_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride,
                          uint64_t frames, uint32_t n_fft, uint32_t hop, uint32_t n_mels, const void* d_window,
                          const void* d_basis, const void* d_fb, int log_mode, float floor, void* d_out, uint64_t out_frames,
                          void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_window, 4}, {d_basis, 4}, {d_fb, 4}, {d_out, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (n_fft < ALAC_FEATURES_MIN_NFFT || n_fft > ALAC_FEATURES_MAX_NFFT || hop < 1 || hop > n_fft || n_mels < 1 ||
        n_mels > ALAC_FEATURES_MAX_MELS || channels == 0)
        return ALACGPU_ERR_BAD_ARG;
    if (!(floor > 0.0f) || !std::isfinite(floor)) return ALACGPU_ERR_BAD_ARG;
    if (log_mode != ALAC_FEATURES_LOG_NONE && log_mode != ALAC_FEATURES_LOG_LN && log_mode != ALAC_FEATURES_LOG_10) return ALACGPU_ERR_BAD_ARG;
    if (frames <= n_fft / 2u || frames > src_stride || frames > (1ull << 62) || out_frames != 1u + frames / hop) return ALACGPU_ERR_BAD_ARG;
    alac_features_params p;
    p.log_mode = (uint32_t)log_mode;
    p.floor = floor;
    return launch_stft_mel(ctx, (const void*)alac_logmel_kernel, p, 0u, d_src, rows, channels, src_stride, frames, n_fft, n_fft, hop,
                           n_mels, d_window, d_basis, d_fb, d_out, out_frames, hip_stream);
}

int alacgpu_fbank_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride, uint64_t frames,
                         uint32_t win_length, uint32_t n_fft, uint32_t hop, uint32_t n_mels, const void* d_window, const void* d_basis,
                         const void* d_fb, uint32_t flags, float preemphasis, float scale, void* d_out, uint64_t out_frames,
                         void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_window, 4}, {d_basis, 4}, {d_fb, 4}, {d_out, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (win_length < ALAC_FBANK_MIN_WIN || win_length > ALAC_FBANK_MAX_WIN || n_fft < win_length || n_fft > ALAC_FBANK_MAX_NFFT ||
        hop < 1 || hop > win_length || n_mels < 1 || n_mels > ALAC_FEATURES_MAX_MELS || channels == 0 || (flags & ~(uint32_t)ALAC_FBANK_FLAGS))
        return ALACGPU_ERR_BAD_ARG;
    if (!(preemphasis >= 0.0f && preemphasis <= 1.0f) || !std::isfinite(scale) || scale == 0.0f) return ALACGPU_ERR_BAD_ARG;
    if (frames < 1 || frames > src_stride || frames > (1ull << 61) ||
        out_frames != alac_fbank_frames(frames, win_length, hop, (flags & ALAC_FBANK_SNIP_EDGES) != 0u))
        return ALACGPU_ERR_BAD_ARG;
    alac_fbank_params p;
    p.flags = flags;
    p.preemphasis = preemphasis;
    p.scale = scale;
    return launch_stft_mel(ctx, (const void*)alac_fbank_kernel, p, ALAC_FBANK_LDS_EXTRA, d_src, rows, channels, src_stride, frames,
                           win_length, n_fft, hop, n_mels, d_window, d_basis, d_fb, d_out, out_frames, hip_stream);
}

int alacgpu_mfcc_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride, uint64_t frames,
                        uint32_t win_length, uint32_t n_fft, uint32_t hop, uint32_t n_mels, uint32_t n_ceps, const void* d_window,
                        const void* d_basis, const void* d_fb, const void* d_dct, const void* d_lifter, uint32_t flags,
                        float preemphasis, float scale, float energy_floor, void* d_out, uint64_t out_frames, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_window, 4}, {d_basis, 4}, {d_fb, 4}, {d_dct, 4}, {d_lifter, 4}, {d_out, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (win_length < ALAC_FBANK_MIN_WIN || win_length > ALAC_FBANK_MAX_WIN || n_fft < win_length || n_fft > ALAC_FBANK_MAX_NFFT ||
        hop < 1 || hop > win_length || n_mels < 1 || n_mels > ALAC_FEATURES_MAX_MELS || n_ceps < 1 || n_ceps > n_mels || channels == 0 ||
        (flags & ~(uint32_t)ALAC_MFCC_FLAGS) || ((flags & ALAC_MFCC_RAW_ENERGY) && !(flags & ALAC_MFCC_USE_ENERGY)))
        return ALACGPU_ERR_BAD_ARG;
    if (!(preemphasis >= 0.0f && preemphasis <= 1.0f) || !std::isfinite(scale) || scale == 0.0f || !(energy_floor >= 0.0f) ||
        !std::isfinite(energy_floor))
        return ALACGPU_ERR_BAD_ARG;
    if (frames < 1 || frames > src_stride || frames > (1ull << 61) ||
        out_frames != alac_fbank_frames(frames, win_length, hop, (flags & ALAC_FBANK_SNIP_EDGES) != 0u))
        return ALACGPU_ERR_BAD_ARG;
    alac_mfcc_params p;
    p.dct = (const float*)d_dct;
    p.lifter = (const float*)d_lifter;
    p.n_ceps = n_ceps;
    p.flags = flags;
    p.preemphasis = preemphasis;
    p.scale = scale;
    p.log_energy_floor = energy_floor > 0.0f ? (float)std::log((double)energy_floor) : -INFINITY;   // (rounded once, as mfcc.py's)
    return launch_stft_mel(ctx, (const void*)alac_mfcc_kernel, p, ALAC_MFCC_LDS_EXTRA, d_src, rows, channels, src_stride, frames,
                           win_length, n_fft, hop, n_mels, d_window, d_basis, d_fb, d_out, out_frames, hip_stream);
}

int alacgpu_deltas_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint32_t n_feats,
                          uint64_t src_stride, uint64_t out_stride, uint64_t line_len, const void* d_lengths, uint32_t order,
                          uint32_t window, const void* d_scales, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}, {d_lengths, 8, false}, {d_scales, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || n_feats == 0 || (uint64_t)channels * n_feats > 0xFFFFFFFFull / (ALAC_DELTAS_MAX_ORDER + 1u) || line_len == 0 ||
        line_len > src_stride || line_len > out_stride || order < 1 || order > ALAC_DELTAS_MAX_ORDER || window < 1 ||
        window > ALAC_DELTAS_MAX_WINDOW)
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t lines = (uint64_t)rows * channels * n_feats;
    uint64_t extent, out_extent;
    if (!planes_extent(lines, src_stride, line_len, extent) || !planes_extent(lines * (order + 1u), out_stride, line_len, out_extent) ||
        !apart(d_src, extent, d_out, out_extent))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t tiles = (line_len + ALAC_DELTAS_TILE - 1u) / ALAC_DELTAS_TILE;
    const uint64_t groups = (lines + ALAC_DELTAS_LINES - 1u) / ALAC_DELTAS_LINES;
    if (tiles > 0x7FFFFFFFull || groups > 0x7FFFFFFFull || tiles * groups > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_deltas_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.lengths = (const int64_t*)d_lengths;
    p.scales = (const float*)d_scales;
    p.lines = lines;
    p.src_stride = src_stride;
    p.out_stride = out_stride;
    p.line_len = line_len;
    p.lines_per_row = channels * n_feats;
    p.n_feats = n_feats;
    p.order = order;
    p.window = window;
    p.tiles = (uint32_t)tiles;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_deltas_kernel, dim3((uint32_t)(tiles * groups)), dim3(ALAC_DELTAS_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_normalize_meanvar_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                     uint64_t line_stride, uint64_t line_len, const void* d_valid, int centre, int scale, float eps,
                                     void* hip_stream) {
    uint64_t lines;
    if (!normalize_args_ok(ctx, d_src, d_out, rows, lines_per_row, line_stride, line_len, lines) || !args_ok({{d_valid, 8, false}}))
        return ALACGPU_ERR_BAD_ARG;
    if (!(eps >= 0.0f) || !std::isfinite(eps) || (!centre && !scale)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t grid = alac_meanvar_grid(lines, line_len);
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_meanvar_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.lines = lines;
    p.lines_per_row = lines_per_row;
    p.line_stride = line_stride;
    p.line_len = line_len;
    p.centre = centre ? 1u : 0u;
    p.scale = scale ? 1u : 0u;
    p.eps = eps;
    const bool wave = line_len <= ALAC_NORM_WAVE_MAX;
    const void* const kernel = wave ? (const void*)alac_meanvar_wave_kernel
                                    : line_len <= ALAC_NORM_LDS_MAX ? (const void*)alac_meanvar_lds_kernel : (const void*)alac_meanvar_mem_kernel;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((uint32_t)grid), dim3(wave ? ALAC_NORM_WAVE_THREADS : ALAC_NORM_LINE_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_normalize_top_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                 uint64_t line_stride, uint64_t line_len, float top, float scale, float offset, int relative,
                                 void* hip_stream) {
    uint64_t lines;
    if (!normalize_args_ok(ctx, d_src, d_out, rows, lines_per_row, line_stride, line_len, lines)) return ALACGPU_ERR_BAD_ARG;
    if (!(top >= 0.0f) || !std::isfinite(top) || !std::isfinite(scale) || !std::isfinite(offset)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t row_elems = (uint64_t)lines_per_row * line_len;      // (at most the extent: it fits)
    const uint32_t parts = alac_top_parts(row_elems);
    const uint64_t grid = (uint64_t)rows * parts;
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t need = sizeof(float) * (size_t)grid;
    scratch_hold hold{ctx->norm, stream};
    int rc = ctx->norm.acquire(ctx, stream, need, align_up(need + need / 4, 4096));
    if (rc) return rc;
    alac_top_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.maxima = (float*)ctx->norm.buf[0];
    p.lines_per_row = lines_per_row;
    p.line_stride = line_stride;
    p.line_len = line_len;
    p.row_elems = row_elems;
    p.part_elems = alac_top_part_elems(row_elems);
    p.parts = parts;
    p.top = top;
    p.scale = scale;
    p.offset = offset;
    p.relative = relative ? 1u : 0u;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_top_reduce_kernel, dim3((uint32_t)grid), dim3(ALAC_TOP_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_top_apply_kernel, dim3((uint32_t)grid), dim3(ALAC_TOP_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ctx->norm.release(ctx, stream);
}

int alacgpu_normalize_sliding_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                     uint64_t line_stride, uint64_t line_len, const void* d_valid, uint32_t window, uint32_t min_window,
                                     int center, int norm_vars, void* hip_stream) {
    uint64_t lines;
    if (!normalize_args_ok(ctx, d_src, d_out, rows, lines_per_row, line_stride, line_len, lines) || !args_ok({{d_valid, 8, false}}))
        return ALACGPU_ERR_BAD_ARG;
    if (window < 1 || window > 0x7FFFFFFFu || min_window < 1 || min_window > window) return ALACGPU_ERR_BAD_ARG;
    if (line_len > ALAC_SLIDING_LDS_MAX && window > ALAC_SLIDING_RING_WINDOW_MAX) return ALACGPU_ERR_BAD_ARG;
    const uint64_t grid = alac_sliding_grid(lines, line_len);
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool wave = line_len <= ALAC_SLIDING_WAVE_MAX;
    const void* const kernel = wave ? (const void*)alac_sliding_wave_kernel : (const void*)alac_sliding_line_kernel;
    const size_t lds = alac_sliding_lds_bytes(line_len);          // (at most 68 KiB and a few bytes)
    if (lds > 32768u) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    alac_sliding_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.lines = lines;
    p.lines_per_row = lines_per_row;
    p.line_stride = line_stride;
    p.line_len = line_len;
    p.window = window;
    p.min_window = min_window;
    p.center = center ? 1u : 0u;
    p.norm_vars = norm_vars ? 1u : 0u;
    p.ring = alac_sliding_ring(line_len);
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((uint32_t)grid), dim3(wave ? ALAC_SLIDING_WAVE_THREADS : ALAC_SLIDING_LINE_THREADS), kargs, lds,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_pcen_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row, uint64_t line_stride,
                        uint64_t line_len, const void* d_valid, float b, float gain, float bias, float power, float bias_pow, float eps,
                        float scale, const void* d_table, uint32_t lines_per_param, int stage, void* hip_stream) {
    uint64_t lines;
    if (!normalize_args_ok(ctx, d_src, d_out, rows, lines_per_row, line_stride, line_len, lines) ||
        !args_ok({{d_valid, 8, false}, {d_table, 4, false}}))
        return ALACGPU_ERR_BAD_ARG;
    if (stage != 0 && stage != 1) return ALACGPU_ERR_BAD_ARG;
    if (!(eps > 0.0f) || !std::isfinite(eps) || !(scale > 0.0f) || !std::isfinite(scale)) return ALACGPU_ERR_BAD_ARG;
    if (d_table) {
        if (lines_per_param == 0 || lines_per_row % lines_per_param != 0) return ALACGPU_ERR_BAD_ARG;
    } else if (!(b > 0.0f && b <= 1.0f) || !(gain >= 0.0f) || !std::isfinite(gain) || !(bias >= 0.0f) || !std::isfinite(bias) ||
               !(power > 0.0f) || !std::isfinite(power) || !(bias_pow >= 0.0f) || !std::isfinite(bias_pow)) {
        return ALACGPU_ERR_BAD_ARG;
    }
    const uint64_t grid = alac_pcen_grid(lines, line_len);
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool wave = line_len <= ALAC_PCEN_WAVE_MAX;
    const void* const kernel = wave ? (const void*)alac_pcen_wave_kernel : (const void*)alac_pcen_line_kernel;
    alac_pcen_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.table = (const float*)d_table;
    p.lines = lines;
    p.lines_per_row = lines_per_row;
    p.lines_per_param = d_table ? lines_per_param : 1u;
    p.line_stride = line_stride;
    p.line_len = line_len;
    p.b = b;
    p.gain = gain;
    p.bias = bias;
    p.power = power;
    p.bias_pow = bias_pow;
    p.eps = eps;
    p.scale = scale;
    p.stage = (uint32_t)stage;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((uint32_t)grid), dim3(wave ? ALAC_PCEN_WAVE_THREADS : ALAC_PCEN_LINE_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_vad_energy_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint64_t row_stride, uint64_t line, uint64_t line_len,
                              const void* d_valid, float energy_threshold, float energy_mean_scale, uint32_t frames_context,
                              float proportion_threshold, void* d_mask, uint64_t mask_stride, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_valid, 8, false}, {d_mask, 1}})) return ALACGPU_ERR_BAD_ARG;
    if (line_len == 0 || line_len > mask_stride || line > row_stride || line_len > row_stride - line) return ALACGPU_ERR_BAD_ARG;
    if (!std::isfinite(energy_threshold) || !std::isfinite(energy_mean_scale) || !(energy_mean_scale >= 0.0f) ||
        frames_context > ALAC_VAD_MAX_CONTEXT || !(proportion_threshold >= 0.0f && proportion_threshold <= 1.0f))
        return ALACGPU_ERR_BAD_ARG;
    uint64_t extent;
    if (!planes_extent(rows, row_stride, line + line_len, extent) || mask_stride > (1ull << 60) / std::max<uint64_t>(rows, 1u)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t mask_extent = rows ? (rows - 1u) * mask_stride + line_len : 0u;
    if (!apart(d_src, extent, d_mask, mask_extent)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t grid = alac_vad_grid(rows, line_len);
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_vad_params p;
    p.energy = (const float*)d_src + line;
    p.valid = (const int64_t*)d_valid;
    p.mask = (uint8_t*)d_mask;
    p.rows = rows;
    p.row_stride = row_stride;
    p.line_len = line_len;
    p.mask_stride = mask_stride;
    p.threshold = energy_threshold;
    p.mean_scale = energy_mean_scale;
    p.proportion = proportion_threshold;
    p.context = frames_context;
    const bool wave = line_len <= ALAC_VAD_WAVE_MAX;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(wave ? (const void*)alac_vad_wave_kernel : (const void*)alac_vad_line_kernel, dim3((uint32_t)grid),
                                 dim3(wave ? ALAC_VAD_WAVE_THREADS : ALAC_VAD_LINE_THREADS), kargs, 0, (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_select_frames_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t lines_per_row,
                                 uint64_t line_stride, uint64_t line_len, const void* d_valid, const void* d_mask, uint64_t mask_stride,
                                 void* d_new_lengths, void* hip_stream) {
    uint64_t lines;
    if (!normalize_args_ok(ctx, d_src, d_out, rows, lines_per_row, line_stride, line_len, lines) ||
        !args_ok({{d_valid, 8, false}, {d_mask, 1}, {d_new_lengths, 8}}))
        return ALACGPU_ERR_BAD_ARG;
    if (line_len > mask_stride || mask_stride > (1ull << 60) / std::max<uint64_t>(rows, 1u)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t extent = lines ? sizeof(float) * ((lines - 1u) * line_stride + line_len) : 0u;
    const uint64_t mask_extent = rows ? (rows - 1u) * mask_stride + line_len : 0u, lengths_extent = sizeof(int64_t) * (uint64_t)rows;
    if (!apart(d_mask, mask_extent, d_src, extent) || !apart(d_mask, mask_extent, d_out, extent) ||
        !apart(d_new_lengths, lengths_extent, d_src, extent) || !apart(d_new_lengths, lengths_extent, d_out, extent) ||
        !apart(d_new_lengths, lengths_extent, d_mask, mask_extent))
        return ALACGPU_ERR_BAD_ARG;
    // new lengths over the old ones: a row's length may then be read by one workgroup only, the one that writes it
    const bool over = d_valid && d_new_lengths == d_valid;
    if (d_valid && !over && !apart(d_new_lengths, lengths_extent, d_valid, lengths_extent)) return ALACGPU_ERR_BAD_ARG;
    const uint32_t groups = over ? 1u : (lines_per_row + ALAC_SELECT_LINES - 1u) / ALAC_SELECT_LINES;
    if ((uint64_t)rows * groups > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_select_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.mask = (const uint8_t*)d_mask;
    p.new_lengths = (int64_t*)d_new_lengths;
    p.lines_per_row = lines_per_row;
    p.groups = groups;
    p.line_stride = line_stride;
    p.line_len = line_len;
    p.mask_stride = mask_stride;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_select_frames_kernel, dim3(rows * groups), dim3(ALAC_SELECT_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_specaugment_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint32_t n_mels,
                               uint64_t line_stride, uint64_t line_len, const void* d_valid, const void* d_warp, const void* d_freq,
                               uint32_t n_freq, const void* d_time, uint32_t n_time, float fill, void* hip_stream) {
    uint64_t lines;
    if (channels == 0 || n_mels == 0 || (uint64_t)channels * n_mels > 0xFFFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (!normalize_args_ok(ctx, d_src, d_out, rows, channels * n_mels, line_stride, line_len, lines) ||
        !args_ok({{d_valid, 8, false}, {d_warp, 4, false}, {d_freq, 4, n_freq != 0}, {d_time, 4, n_time != 0}}))
        return ALACGPU_ERR_BAD_ARG;
    if (!std::isfinite(fill) || n_freq > ALAC_AUG_MAX_MASKS || n_time > ALAC_AUG_MAX_MASKS || (d_warp && line_len > ALAC_AUG_LDS_MAX))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t grid = alac_augment_grid(lines, line_len);
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool wave = line_len <= ALAC_AUG_WAVE_MAX;
    const void* const kernel = wave ? (const void*)alac_specaugment_wave_kernel : (const void*)alac_specaugment_line_kernel;
    const size_t lds = alac_augment_lds_bytes(line_len, n_time, d_warp != nullptr);      // (at most 72 KiB by the limits above)
    if (lds > 32768u) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    alac_augment_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.warp = (const int32_t*)d_warp;
    p.freq = (const int32_t*)d_freq;
    p.time = (const int32_t*)d_time;
    p.lines = lines;
    p.lines_per_row = channels * n_mels;
    p.n_mels = n_mels;
    p.n_freq = n_freq;
    p.n_time = n_time;
    p.stage = d_warp ? (uint32_t)line_len : 0u;
    p.line_stride = line_stride;
    p.line_len = line_len;
    p.fill = fill;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((uint32_t)grid), dim3(ALAC_AUG_THREADS), kargs, lds, (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_reverb_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, const void* d_rir, uint32_t rows, uint32_t channels,
                          uint32_t rir_channels, uint64_t stride, uint64_t rir_stride, uint64_t frames, uint64_t rir_frames,
                          const void* d_valid, const void* d_rir_valid, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}, {d_rir, 4}, {d_valid, 8, false}, {d_rir_valid, 8, false}})) return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || (rir_channels != 1u && rir_channels != channels) || frames == 0 || frames > stride || rir_frames == 0 ||
        rir_frames > rir_stride)
        return ALACGPU_ERR_BAD_ARG;
    uint64_t extent, rir_extent;
    if (!planes_extent((uint64_t)rows * channels, stride, frames, extent) ||
        !planes_extent((uint64_t)rows * rir_channels, rir_stride, rir_frames, rir_extent))
        return ALACGPU_ERR_BAD_ARG;
    if ((d_src != d_out && !apart(d_src, extent, d_out, extent)) || !apart(d_rir, rir_extent, d_out, extent)) return ALACGPU_ERR_BAD_ARG;
    // (frames and rir_frames are below 2^58: the sums fit)
    const uint64_t x_blocks = alac_reverb_x_blocks(frames), parts = alac_reverb_parts(rir_frames);
    const uint64_t out_blocks = alac_reverb_out_blocks(frames, rir_frames);
    if (x_blocks > 0x7FFFFFFFull / channels || parts > 0x7FFFFFFFull / rir_channels || out_blocks > 0x7FFFFFFFull / channels)
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t units = channels * x_blocks + rir_channels * parts + 1u;
    if (units * std::max<uint64_t>(rows, 1u) > 0x7FFFFFFFull || out_blocks * channels * std::max<uint64_t>(rows, 1u) > 0x7FFFFFFFull)
        return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t spectra = sizeof(float2) * ALAC_REVERB_N * (size_t)(units - 1u) * rows;
    const size_t need = spectra + sizeof(alac_reverb_row) * (size_t)rows;
    scratch_hold hold{ctx->reverb, stream};
    int rc = ctx->reverb.acquire(ctx, stream, need, align_up(need + need / 4, 4096));
    if (rc) return rc;
    if (!ctx->d_reverb_twiddles) {
        // once per ctx: exp(-2 pi i k / N) in double, rounded once, in page-locked memory of the ctx and copied on the call's own
        // stream in front of its launches -- a synchronous copy would hold the host behind whatever else the device is busy with
        if (!ctx->h_reverb_twiddles) HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_reverb_twiddles, sizeof(float2) * ALAC_REVERB_N));
        float2* const table = (float2*)ctx->h_reverb_twiddles;
        for (uint32_t k = 0; k < ALAC_REVERB_N; k++) {
            const double a = 2.0 * 3.14159265358979323846 * (double)k / (double)ALAC_REVERB_N;
            table[k] = make_float2((float)std::cos(a), (float)-std::sin(a));
        }
        void* d_table = nullptr;
        HIP_TRY(ctx, hipMalloc(&d_table, sizeof(float2) * ALAC_REVERB_N));
        const hipError_t e = hipMemcpyAsync(d_table, table, sizeof(float2) * ALAC_REVERB_N, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) {
            (void)hipFree(d_table);
            HIP_TRY(ctx, e);
        }
        ctx->d_reverb_twiddles = d_table;     // (a later call on another stream waits for this call's event, so for the copy)
    }
    alac_reverb_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.rir = (const float*)d_rir;
    p.valid = (const int64_t*)d_valid;
    p.rir_valid = (const int64_t*)d_rir_valid;
    p.twiddles = (const float2*)ctx->d_reverb_twiddles;
    p.spectra = (float2*)ctx->reverb.buf[0];
    p.verdict = (alac_reverb_row*)((char*)ctx->reverb.buf[0] + spectra);
    p.channels = channels;
    p.rir_channels = rir_channels;
    p.stride = stride;
    p.rir_stride = rir_stride;
    p.frames = frames;
    p.rir_frames = rir_frames;
    p.x_blocks = (uint32_t)x_blocks;
    p.rir_parts = (uint32_t)parts;
    p.units = (uint32_t)units;
    p.out_blocks = (uint32_t)out_blocks;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_reverb_analyse_kernel, dim3((uint32_t)(units * rows)), dim3(ALAC_REVERB_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_reverb_synth_kernel, dim3((uint32_t)(out_blocks * channels * rows)), dim3(ALAC_REVERB_THREADS),
                                 kargs, 0, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ctx->reverb.release(ctx, stream);
}

int alacgpu_rir_shoebox_device(alacgpu_ctx* ctx, const void* d_geometry, const void* d_beta, uint32_t rows, uint32_t sample_rate,
                               uint64_t frames, uint32_t taps, int32_t max_order, double sound_speed, void* d_out, uint64_t out_stride,
                               void* d_lengths, void* hip_stream) {
    if (!ctx || !args_ok({{d_geometry, 8}, {d_beta, 4}, {d_out, 4}, {d_lengths, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (sample_rate == 0 || sample_rate > 0x7FFFFFFFu || frames == 0 || frames > ALAC_RIR_MAX_FRAMES || frames > out_stride || taps < 3u ||
        taps > ALAC_RIR_MAX_TAPS || taps % 2u == 0u || max_order < -1 || !(sound_speed > 0.0) || !std::isfinite(sound_speed))
        return ALACGPU_ERR_BAD_ARG;
    uint64_t extent, geometry_extent, beta_extent, lengths_extent;
    if (!planes_extent(rows, out_stride, frames, extent) || !planes_extent(rows, 18u, 18u, geometry_extent) ||
        !planes_extent(rows, 6u, 6u, beta_extent) || !planes_extent(rows, 1u, 1u, lengths_extent))
        return ALACGPU_ERR_BAD_ARG;
    if (!apart(d_geometry, geometry_extent, d_out, extent) || !apart(d_beta, beta_extent, d_out, extent) ||
        !apart(d_lengths, lengths_extent, d_out, extent) || !apart(d_lengths, lengths_extent, d_geometry, geometry_extent) ||
        !apart(d_lengths, lengths_extent, d_beta, beta_extent))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t tiles = (frames + ALAC_RIR_TILE - 1u) / ALAC_RIR_TILE;
    if (tiles * std::max<uint64_t>(rows, 1u) > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_rir_params p = {};
    p.geometry = (const double*)d_geometry;
    p.beta = (const float*)d_beta;
    p.out = (float*)d_out;
    p.lengths = (int32_t*)d_lengths;
    p.out_stride = out_stride;
    p.frames = (uint32_t)frames;
    p.taps = taps;
    p.tiles = (uint32_t)tiles;
    p.max_order = max_order;
    p.scale = (double)sample_rate / sound_speed;
    p.tw = (float)(2.0 * 3.14159265358979323846 / (double)taps);
    for (uint32_t j = 0; j <= taps / 2u; j++) {      // the window's table, in double and rounded once (rir.window_table)
        const double a = 2.0 * 3.14159265358979323846 * (double)j / (double)taps;
        p.cw[j] = (float)std::cos(a);
        p.sw[j] = (float)std::sin(a);
    }
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_rir_shoebox_kernel, dim3((uint32_t)(tiles * rows)), dim3(ALAC_RIR_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_mix_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, const void* d_noise, uint32_t rows, uint32_t channels,
                       uint32_t noise_channels, uint64_t stride, uint64_t noise_stride, uint64_t frames, const void* d_valid,
                       const void* d_noise_valid, const void* d_ratio, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}, {d_noise, 4}, {d_valid, 8, false}, {d_noise_valid, 8, false}, {d_ratio, 4}}))
        return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || (noise_channels != 1u && noise_channels != channels) || frames == 0 || frames > stride || frames > noise_stride)
        return ALACGPU_ERR_BAD_ARG;
    uint64_t extent, noise_extent;
    if (!planes_extent((uint64_t)rows * channels, stride, frames, extent) ||
        !planes_extent((uint64_t)rows * noise_channels, noise_stride, frames, noise_extent))
        return ALACGPU_ERR_BAD_ARG;
    if ((d_src != d_out && !apart(d_src, extent, d_out, extent)) || !apart(d_noise, noise_extent, d_out, extent)) return ALACGPU_ERR_BAD_ARG;
    const uint32_t parts = alac_mix_parts(frames);
    const uint64_t grid = (uint64_t)rows * parts;
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t need = 2u * sizeof(float) * (size_t)grid;
    scratch_hold hold{ctx->mix, stream};
    int rc = ctx->mix.acquire(ctx, stream, need, align_up(need + need / 4, 4096));
    if (rc) return rc;
    const auto wide = [](const void* base, uint64_t plane_stride) { return ((uintptr_t)base & 15u) == 0u && (plane_stride & 3u) == 0u; };
    alac_mix_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.noise = (const float*)d_noise;
    p.valid = (const int64_t*)d_valid;
    p.noise_valid = (const int64_t*)d_noise_valid;
    p.ratio = (const float*)d_ratio;
    p.sums = (float*)ctx->mix.buf[0];
    p.channels = channels;
    p.noise_channels = noise_channels;
    p.stride = stride;
    p.noise_stride = noise_stride;
    p.frames = frames;
    p.part_frames = alac_mix_part_frames(frames);
    p.parts = parts;
    p.vec = wide(d_src, stride) && wide(d_out, stride) ? 1u : 0u;
    p.noise_vec = wide(d_noise, noise_stride) ? 1u : 0u;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_mix_reduce_kernel, dim3((uint32_t)grid), dim3(ALAC_MIX_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_mix_apply_kernel, dim3((uint32_t)grid), dim3(ALAC_MIX_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ctx->mix.release(ctx, stream);
}

int alacgpu_biquad_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint64_t stride,
                          uint64_t frames, const void* d_valid, const void* d_coeffs, uint32_t sections, const void* d_gain, int clamp,
                          void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}, {d_valid, 8, false}, {d_coeffs, 8}, {d_gain, 8, false}})) return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || sections == 0 || sections > ALAC_BIQUAD_MAX_SECTIONS || frames == 0 || frames > stride) return ALACGPU_ERR_BAD_ARG;
    uint64_t extent;
    if (!planes_extent((uint64_t)rows * channels, stride, frames, extent)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t coeff_bytes = sizeof(double) * 5u * (uint64_t)sections * rows, gain_bytes = d_gain ? sizeof(double) * (uint64_t)rows : 0u;
    if ((d_src != d_out && !apart(d_src, extent, d_out, extent)) || !apart(d_coeffs, coeff_bytes, d_out, extent) ||
        (d_gain && !apart(d_gain, gain_bytes, d_out, extent)))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t grid = (uint64_t)rows * channels;
    if (grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_biquad_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.coeffs = (const double*)d_coeffs;
    p.gain = (const double*)d_gain;
    p.channels = channels;
    p.sections = sections;
    p.stride = stride;
    p.frames = frames;
    p.clamp = clamp ? 1u : 0u;
    p.vec = ((uintptr_t)d_src & 15u) == 0u && ((uintptr_t)d_out & 15u) == 0u && (stride & 3u) == 0u ? 1u : 0u;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_biquad_kernel, dim3((uint32_t)grid), dim3(ALAC_BIQUAD_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_level_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint64_t stride,
                         uint64_t frames, const void* d_valid, uint32_t mode, uint32_t hop, const void* d_kweight, double target,
                         double max_peak, int clamp, void* d_gain_out, void* d_energy_out, void* d_peak_out, void* hip_stream) {
    const bool lufs = mode == ALAC_LEVEL_LUFS;
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4, false}, {d_valid, 8, false}, {d_kweight, 8, lufs}, {d_gain_out, 8, false},
                          {d_energy_out, 8, false}, {d_peak_out, 8, false}}))
        return ALACGPU_ERR_BAD_ARG;
    if (!d_out && !d_gain_out && !d_energy_out && !d_peak_out) return ALACGPU_ERR_BAD_ARG;      // (nothing asked for)
    if (mode > ALAC_LEVEL_LUFS || channels == 0 || (lufs && (channels > ALAC_LEVEL_MAX_CHANNELS || hop < ALAC_LEVEL_MIN_HOP)) ||
        frames == 0 || frames > stride || !(target > 0.0) || !std::isfinite(target) || !std::isfinite(max_peak))
        return ALACGPU_ERR_BAD_ARG;
    uint64_t extent;
    if (!planes_extent((uint64_t)rows * channels, stride, frames, extent)) return ALACGPU_ERR_BAD_ARG;
    if (d_out && d_src != d_out && !apart(d_src, extent, d_out, extent)) return ALACGPU_ERR_BAD_ARG;
    const uint64_t per_row = sizeof(double) * (uint64_t)rows;
    for (const void* o : {(const void*)d_gain_out, (const void*)d_energy_out, (const void*)d_peak_out})
        if (o && (!apart(o, per_row, d_src, extent) || (d_out && !apart(o, per_row, d_out, extent)))) return ALACGPU_ERR_BAD_ARG;
    if (lufs && d_out && !apart(d_kweight, sizeof(double) * 10u, d_out, extent)) return ALACGPU_ERR_BAD_ARG;
    const uint32_t parts = d_out ? alac_level_parts(frames) : 1u;
    const uint64_t planes = (uint64_t)rows * channels, grid = (uint64_t)rows * parts;
    if (planes > 0x7FFFFFFFull || grid > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const uint64_t hops = alac_level_hops(mode, frames, hop);
    const size_t need = sizeof(double) * (size_t)(planes * (ALAC_LEVEL_HEAD + hops));      // (below the signal's own extent and 2^36)
    scratch_hold hold{ctx->level, stream};
    int rc = ctx->level.acquire(ctx, stream, need, align_up(need + need / 4, 4096));
    if (rc) return rc;
    alac_level_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.kweight = (const double*)d_kweight;
    p.scratch = (double*)ctx->level.buf[0];
    p.gain_out = (double*)d_gain_out;
    p.energy_out = (double*)d_energy_out;
    p.peak_out = (double*)d_peak_out;
    p.target = target;
    p.max_peak = max_peak;
    p.stride = stride;
    p.frames = frames;
    p.hops = hops;
    p.part_frames = alac_level_part_frames(frames);
    p.channels = channels;
    p.mode = mode;
    p.hop = lufs ? hop : 1u;
    p.parts = parts;
    p.clamp = clamp ? 1u : 0u;
    p.vec = ((uintptr_t)d_src & 15u) == 0u && (stride & 3u) == 0u ? 1u : 0u;
    p.vec_out = p.vec && ((uintptr_t)d_out & 15u) == 0u ? 1u : 0u;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_level_measure_kernel, dim3((uint32_t)planes), dim3(ALAC_LEVEL_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_level_apply_kernel, dim3((uint32_t)grid), dim3(ALAC_LEVEL_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ctx->level.release(ctx, stream);
}

int alacgpu_time_stretch_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint64_t src_stride,
                                uint64_t out_stride, uint64_t frames, uint64_t out_frames, const void* d_p, const void* d_q,
                                const void* d_valid, void* d_valid_out, uint32_t n_fft, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}, {d_p, 4}, {d_q, 4}, {d_valid, 8, false}, {d_valid_out, 8}})) return ALACGPU_ERR_BAD_ARG;
    const int which = n_fft == 512u ? 0 : n_fft == 1024u ? 1 : n_fft == 2048u ? 2 : -1;
    if (which < 0 || channels == 0 || frames == 0 || frames > src_stride || out_frames == 0 || out_frames > out_stride ||
        frames >= (1ull << 40) || out_frames >= (1ull << 40))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t planes = (uint64_t)rows * channels;
    uint64_t extent, out_extent;
    if (!planes_extent(planes, src_stride, frames, extent) || !planes_extent(planes, out_stride, out_frames, out_extent))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t terms = sizeof(int32_t) * (uint64_t)rows, lens = sizeof(int64_t) * (uint64_t)rows;
    if (!apart(d_src, extent, d_out, out_extent) || !apart(d_p, terms, d_out, out_extent) || !apart(d_q, terms, d_out, out_extent) ||
        !apart(d_valid_out, lens, d_out, out_extent) || !apart(d_valid_out, lens, d_src, extent) || !apart(d_valid_out, lens, d_p, terms) ||
        !apart(d_valid_out, lens, d_q, terms) || (d_valid && (!apart(d_valid, lens, d_out, out_extent) || !apart(d_valid, lens, d_valid_out, lens))))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t bins = n_fft / 2u + 1u, t_max = alac_stretch_frames(frames, n_fft), t_cap = alac_stretch_cap(out_frames, n_fft);
    const uint64_t tiles = alac_stretch_tiles(out_frames, n_fft), many = std::max<uint64_t>(planes, 1u);
    if (planes > 0x7FFFFFFFull || t_max > 0x7FFFFFFFull / many || tiles > 0x7FFFFFFFull / many || t_cap > 0x7FFFFFFFull ||
        planes * bins > 0x7FFFFFFFull * (uint64_t)ALAC_STRETCH_SCAN_THREADS)
        return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t need_x = sizeof(float2) * (size_t)(planes * t_max * bins), need_y = sizeof(float2) * (size_t)(planes * t_cap * bins);
    scratch_hold hold{ctx->stretch, stream};
    int rc = ctx->stretch.acquire(ctx, stream, need_x, align_up(need_x + need_x / 4, 4096), need_y, align_up(need_y + need_y / 4, 4096));
    if (rc) return rc;
    const size_t table_bytes = (sizeof(float2) + sizeof(float)) * (size_t)n_fft;
    if (!ctx->d_stretch_tables[which]) {
        // once per ctx and n_fft: the twiddles and the window in double, rounded once, in page-locked memory of the ctx and copied
        // on the call's own stream in front of its launches (as alacgpu_reverb_device's table is)
        if (!ctx->h_stretch_tables[which]) HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_stretch_tables[which], table_bytes));
        float2* const table = (float2*)ctx->h_stretch_tables[which];
        float* const window = (float*)(table + n_fft);
        for (uint32_t k = 0; k < n_fft; k++) {
            const double a = 2.0 * 3.14159265358979323846 * (double)k / (double)n_fft;
            table[k] = make_float2((float)std::cos(a), (float)-std::sin(a));
            window[k] = (float)(0.5 - 0.5 * std::cos(a));
        }
        void* d_table = nullptr;
        HIP_TRY(ctx, hipMalloc(&d_table, table_bytes));
        const hipError_t e = hipMemcpyAsync(d_table, table, table_bytes, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) {
            (void)hipFree(d_table);
            HIP_TRY(ctx, e);
        }
        ctx->d_stretch_tables[which] = d_table;   // (a later call on another stream waits for this call's event, so for the copy)
    }
    alac_stretch_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.p = (const int32_t*)d_p;
    p.q = (const int32_t*)d_q;
    p.valid = (const int64_t*)d_valid;
    p.valid_out = (int64_t*)d_valid_out;
    p.table = (const float2*)ctx->d_stretch_tables[which];
    p.window = (const float*)(p.table + n_fft);
    p.X = (float2*)ctx->stretch.buf[0];
    p.Y = (float2*)ctx->stretch.buf[1];
    p.src_stride = src_stride;
    p.out_stride = out_stride;
    p.frames = frames;
    p.out_frames = out_frames;
    p.chains = planes * bins;
    p.channels = channels;
    p.t_max = (uint32_t)t_max;
    p.t_cap = (uint32_t)t_cap;
    p.out_tiles = (uint32_t)tiles;
    const void *analyse, *scan, *synth;
    alac_stretch_kernels(n_fft, analyse, scan, synth);
    const uint32_t threads = alac_stretch_threads(n_fft);
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(analyse, dim3((uint32_t)(planes * t_max)), dim3(threads), kargs, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel(scan, dim3((uint32_t)((p.chains + ALAC_STRETCH_SCAN_THREADS - 1u) / ALAC_STRETCH_SCAN_THREADS)),
                                 dim3(ALAC_STRETCH_SCAN_THREADS), kargs, 0, stream));
    HIP_TRY(ctx, hipLaunchKernel(synth, dim3((uint32_t)(planes * tiles)), dim3(threads), kargs, 0, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ctx->stretch.release(ctx, stream);
}

int alacgpu_copy_rows_device(alacgpu_ctx* ctx, const void* d_src, void* d_out, uint32_t rows, uint32_t channels, uint64_t src_stride,
                             uint64_t out_stride, uint64_t frames, const void* d_valid, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_out, 4}, {d_valid, 8}})) return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || frames == 0 || frames > src_stride || frames > out_stride) return ALACGPU_ERR_BAD_ARG;
    const uint64_t planes = (uint64_t)rows * channels;
    uint64_t extent, out_extent;
    if (!planes_extent(planes, src_stride, frames, extent) || !planes_extent(planes, out_stride, frames, out_extent) ||
        !apart(d_src, extent, d_out, out_extent) || !apart(d_valid, sizeof(int64_t) * (uint64_t)rows, d_out, out_extent))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t tiles = (frames + ALAC_STRETCH_COPY_TILE - 1u) / ALAC_STRETCH_COPY_TILE;
    if (tiles > 0x7FFFFFFFull / std::max<uint64_t>(planes, 1u)) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_copy_rows_params p;
    p.src = (const float*)d_src;
    p.out = (float*)d_out;
    p.valid = (const int64_t*)d_valid;
    p.src_stride = src_stride;
    p.out_stride = out_stride;
    p.frames = frames;
    p.channels = channels;
    p.tiles = (uint32_t)tiles;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_copy_rows_kernel, dim3((uint32_t)(planes * tiles)), dim3(ALAC_STRETCH_COPY_THREADS), kargs, 0,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_yin_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t stride, uint64_t frames,
                       const void* d_valid, uint32_t sample_rate, uint32_t win_length, uint32_t hop, uint32_t tau_min, uint32_t tau_max,
                       uint32_t align_length, float threshold, void* d_out, uint64_t out_frames, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {d_valid, 8, false}, {d_out, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || frames == 0 || frames > stride || sample_rate == 0 || hop == 0) return ALACGPU_ERR_BAD_ARG;
    if (win_length < ALAC_YIN_MIN_WIN || win_length > ALAC_YIN_MAX_WIN || win_length % 64u != 0u || tau_min < 2u ||
        tau_max > ALAC_YIN_MAX_LAG || tau_max <= tau_min + 1u || !(threshold > 0.0f && threshold <= 1.0f))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t expect = align_length ? (frames < align_length ? 0u : 1u + (frames - align_length) / hop) : frames / hop + 1u;
    if (out_frames != expect) return ALACGPU_ERR_BAD_ARG;
    const uint64_t planes = (uint64_t)rows * channels;
    uint64_t extent, out_extent;
    if (!planes_extent(planes, stride, frames, extent) || !planes_extent(planes, 2u * out_frames, 2u * out_frames, out_extent) ||
        !apart(d_src, extent, d_out, out_extent))
        return ALACGPU_ERR_BAD_ARG;
    const uint32_t tile = alac_yin_tile(win_length, tau_max, hop);
    const uint64_t tiles = (out_frames + tile - 1u) / tile;
    if (tiles > 0x7FFFFFFFull || tiles * std::max<uint64_t>(planes, 1u) > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    if (rows == 0 || out_frames == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    alac_yin_params p;
    p.src = (const float*)d_src;
    p.valid = (const int64_t*)d_valid;
    p.out = (float*)d_out;
    p.channels = channels;
    p.stride = stride;
    p.frames = frames;
    p.out_frames = out_frames;
    p.win = win_length;
    p.hop = hop;
    p.tau_min = tau_min;
    p.tau_max = tau_max;
    p.align = align_length;
    p.first = (int64_t)(align_length / 2u) - (int64_t)((win_length + tau_max) / 2u);
    p.tile = tile;
    p.tiles = (uint32_t)tiles;
    p.samples = alac_yin_samples(win_length, tau_max, hop, tile);
    p.threshold = threshold;
    p.rate = (float)sample_rate;
    const size_t lds = sizeof(float) * ((size_t)p.samples + (size_t)tile * (tau_max + 1u));
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(hop % 4u == 0u ? (const void*)alac_yin_kernel_vec : (const void*)alac_yin_kernel,
                                 dim3((uint32_t)(tiles * planes)), dim3(ALAC_YIN_THREADS), kargs, lds, (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_pyin_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t stride, uint64_t frames,
                        const void* d_valid, uint32_t sample_rate, uint32_t win_length, uint32_t hop, uint32_t tau_min, uint32_t tau_max,
                        uint32_t align_length, uint32_t n_thresholds, uint32_t n_bins, uint32_t band, float no_trough_prob,
                        const void* d_table, void* d_obs_voiced, void* d_obs_unvoiced, void* d_vp, void* d_out, void* d_states,
                        uint64_t out_frames, int stage, void* hip_stream) {
    if (!ctx || stage < 0 || stage > 2) return ALACGPU_ERR_BAD_ARG;
    const bool observe = stage != 2, decode = stage != 1;
    if (!args_ok({{d_src, 4, observe}, {d_valid, 8, false}, {d_table, 4}, {d_obs_voiced, 4, stage != 0}, {d_obs_unvoiced, 4, stage != 0},
                  {d_vp, 4, stage == 1}, {d_out, 4, stage == 0}, {d_states, 4, stage == 2}}))
        return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || sample_rate == 0 || hop == 0) return ALACGPU_ERR_BAD_ARG;
    if (win_length < ALAC_YIN_MIN_WIN || win_length > ALAC_YIN_MAX_WIN || win_length % 64u != 0u || tau_min < 2u ||
        tau_max > ALAC_YIN_MAX_LAG || tau_max <= tau_min + 1u)
        return ALACGPU_ERR_BAD_ARG;
    if (n_thresholds < 1u || n_thresholds > ALAC_PYIN_MAX_THRESHOLDS || n_bins < 1u || n_bins > ALAC_PYIN_MAX_BINS || band >= n_bins ||
        !(no_trough_prob >= 0.0f && no_trough_prob <= 1.0f))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t planes = (uint64_t)rows * channels;
    if (planes > 0x7FFFFFFFull || out_frames >= (1ull << 31)) return ALACGPU_ERR_BAD_ARG;
    // the observations (voiced, unvoiced, vp) and the backpointers: in the ctx's scratch where the caller holds neither
    const uint64_t cells = planes * out_frames;
    const uint64_t obs_bytes = sizeof(float) * cells * ((uint64_t)n_bins + 2u), back_bytes = sizeof(uint16_t) * cells * 2u * n_bins;
    if ((stage == 0 ? obs_bytes : 0u) + (decode ? back_bytes : 0u) > (1ull << 31)) return ALACGPU_ERR_BAD_ARG;
    uint32_t tile = 0;
    uint64_t tiles = 0;
    if (observe) {
        if (frames == 0 || frames > stride) return ALACGPU_ERR_BAD_ARG;
        const uint64_t expect = align_length ? (frames < align_length ? 0u : 1u + (frames - align_length) / hop) : frames / hop + 1u;
        if (out_frames != expect) return ALACGPU_ERR_BAD_ARG;
        uint64_t extent, out_extent;
        if (!planes_extent(planes, stride, frames, extent) || !planes_extent(planes, 3u * out_frames, 3u * out_frames, out_extent) ||
            (stage == 0 && !apart(d_src, extent, d_out, out_extent)) ||
            (stage == 1 && (!apart(d_src, extent, d_obs_voiced, sizeof(float) * cells * n_bins) ||
                            !apart(d_src, extent, d_obs_unvoiced, sizeof(float) * cells) || !apart(d_src, extent, d_vp, sizeof(float) * cells))))
            return ALACGPU_ERR_BAD_ARG;
        tile = alac_yin_tile(win_length, tau_max, hop);
        tiles = (out_frames + tile - 1u) / tile;
        if (tiles > 0x7FFFFFFFull || tiles * std::max<uint64_t>(planes, 1u) > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    }
    if (rows == 0 || out_frames == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    scratch_hold hold{ctx->pyin, stream};
    const size_t need_obs = stage == 0 ? (size_t)obs_bytes : 0u, need_back = decode ? (size_t)back_bytes : 0u;
    int rc = ctx->pyin.acquire(ctx, stream, need_obs, align_up(need_obs + need_obs / 4, 4096), need_back, align_up(need_back + need_back / 4, 4096));
    if (rc) return rc;
    const uint32_t K = alac_pyin_max_troughs(tau_min, tau_max);
    const alac_pyin_tables tab = alac_pyin_tables_at((const float*)d_table, n_thresholds, K, n_bins, band);
    float* obs_voiced = (float*)(stage == 0 ? ctx->pyin.buf[0] : d_obs_voiced);
    float* obs_unvoiced = stage == 0 ? obs_voiced + cells * n_bins : (float*)d_obs_unvoiced;
    float* vp = stage == 0 ? obs_unvoiced + cells : (float*)d_vp;
    if (observe) {
        alac_pyin_obs_params q;
        alac_yin_params& p = q.y;
        p.src = (const float*)d_src;
        p.valid = (const int64_t*)d_valid;
        p.out = nullptr;
        p.channels = channels;
        p.stride = stride;
        p.frames = frames;
        p.out_frames = out_frames;
        p.win = win_length;
        p.hop = hop;
        p.tau_min = tau_min;
        p.tau_max = tau_max;
        p.align = align_length;
        p.first = (int64_t)(align_length / 2u) - (int64_t)((win_length + tau_max) / 2u);
        p.tile = tile;
        p.tiles = (uint32_t)tiles;
        p.samples = alac_yin_samples(win_length, tau_max, hop, tile);
        p.threshold = 0.0f;
        p.rate = (float)sample_rate;
        q.tab = tab;
        q.obs_voiced = obs_voiced;
        q.obs_unvoiced = obs_unvoiced;
        q.vp = vp;
        q.n_thresholds = n_thresholds;
        q.n_bins = n_bins;
        q.max_troughs = K;
        q.no_trough = no_trough_prob;
        const size_t lds = sizeof(float) * alac_pyin_obs_lds_floats(p, K, n_bins);
        void* kargs[] = {&q};
        HIP_TRY(ctx, hipLaunchKernel(hop % 4u == 0u ? (const void*)alac_pyin_obs_kernel_vec : (const void*)alac_pyin_obs_kernel,
                                     dim3((uint32_t)(tiles * planes)), dim3(ALAC_YIN_THREADS), kargs, lds, stream));
    }
    if (decode) {
        alac_pyin_decode_params q;
        q.obs_voiced = obs_voiced;
        q.obs_unvoiced = obs_unvoiced;
        q.vp = stage == 0 ? vp : nullptr;
        q.valid = (const int64_t*)d_valid;
        q.back = (uint16_t*)ctx->pyin.buf[1];
        q.out = stage == 0 ? (float*)d_out : nullptr;
        q.states = stage == 2 ? (int32_t*)d_states : nullptr;
        q.tab = tab;
        q.channels = channels;
        q.n_bins = n_bins;
        q.band = band;
        q.frames = frames;
        q.out_frames = out_frames;
        q.hop = hop;
        q.align = align_length;
        q.counts_are_frames = stage == 2 ? 1u : 0u;
        void* kargs[] = {&q};
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_pyin_decode_kernel, dim3((uint32_t)planes), dim3(ALAC_PYIN_DECODE_THREADS), kargs, 0, stream));
    }
    HIP_TRY(ctx, hipGetLastError());
    return ctx->pyin.release(ctx, stream);
}

int alacgpu_kaldi_pitch_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t stride, uint64_t frames,
                               const void* d_valid, uint32_t sample_rate, uint32_t resample_freq, uint32_t win_length, uint32_t hop,
                               uint32_t window, uint32_t shift, uint32_t first_lag, uint32_t last_lag, uint32_t n_states, uint32_t phases,
                               uint32_t in_per_unit, uint32_t down_taps, uint32_t up_taps, uint32_t flags, uint32_t left_context,
                               uint32_t right_context, uint32_t delta_window, const void* d_table, void* d_nccf, void* d_raw, void* d_out,
                               uint64_t out_frames, int stage, void* hip_stream) {
    if (!ctx || stage < 0 || stage > 3) return ALACGPU_ERR_BAD_ARG;
    const bool front = stage <= 1, decode = stage == 0 || stage == 2, process = (flags & ALAC_KPITCH_PROCESS) != 0u;
    const bool epilogue = process && (stage == 0 || stage == 3);
    if (!args_ok({{d_src, 4, front}, {d_valid, 8, false}, {d_table, 4}, {d_nccf, 4, stage == 1 || stage == 2}, {d_raw, 4, stage >= 2},
                  {d_out, 4, stage == 0 || stage == 3}}))
        return ALACGPU_ERR_BAD_ARG;
    if (channels == 0 || sample_rate == 0 || resample_freq == 0 || resample_freq > sample_rate || win_length == 0 || hop == 0 || window < 2u ||
        shift == 0)
        return ALACGPU_ERR_BAD_ARG;
    if (first_lag < 1u || last_lag <= first_lag || n_states < 1u || n_states > ALAC_KPITCH_MAX_STATES || phases == 0 || in_per_unit == 0 ||
        down_taps == 0 || (uint64_t)phases * down_taps > ALAC_KPITCH_MAX_DOWN || up_taps == 0 || up_taps > last_lag - first_lag + 1u ||
        window > (1u << 20) || last_lag > (1u << 20) || alac_kpitch_nccf_lds(window, first_lag, last_lag) > ALAC_KPITCH_MAX_LDS ||
        (flags >> 5) != 0u || (process && alac_kpitch_lines(flags) == 0u) || (stage == 3 && !process) || delta_window < 1u || delta_window > 64u ||
        left_context > (1u << 20) || right_context > (1u << 20))
        return ALACGPU_ERR_BAD_ARG;
    const uint64_t planes = (uint64_t)rows * channels;
    if (planes > 0x7FFFFFFFull || out_frames >= (1ull << 31) || frames >= (1ull << 40)) return ALACGPU_ERR_BAD_ARG;
    alac_kpitch_framing fr{sample_rate, resample_freq, win_length, hop, window, shift};
    const uint32_t lines = alac_kpitch_lines(flags);
    const uint64_t n_max = front ? alac_kpitch_samples(fr, frames) : 0u;
    const uint64_t chunks = std::max<uint64_t>((n_max + ALAC_KPITCH_CHUNK - 1u) / ALAC_KPITCH_CHUNK, 1u);
    const uint64_t groups = (out_frames + ALAC_KPITCH_THREADS / 64 - 1u) / (ALAC_KPITCH_THREADS / 64);
    const alac_kpitch_scratch sc = alac_kpitch_scratch_of(planes, n_max, out_frames, n_states, front, stage == 0, decode,
                                                          (stage == 0 && process) || epilogue);
    if (sc.bytes0 + sc.bytes1 > (1ull << 31)) return ALACGPU_ERR_BAD_ARG;
    if (front) {
        if (frames == 0 || frames > stride || out_frames != alac_kpitch_frames(fr, frames)) return ALACGPU_ERR_BAD_ARG;
        uint64_t extent, out_extent;
        if (!planes_extent(planes, stride, frames, extent)) return ALACGPU_ERR_BAD_ARG;
        out_extent = sizeof(float) * planes * out_frames * (stage == 0 ? (uint64_t)lines : 2ull * n_states);
        if (!apart(d_src, extent, stage == 0 ? d_out : d_nccf, out_extent)) return ALACGPU_ERR_BAD_ARG;
        if (planes * chunks > 0x7FFFFFFFull || planes * std::max<uint64_t>(groups, 1u) > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    }
    const uint64_t cells = sizeof(float) * planes * out_frames;
    if ((stage == 2 && !apart(d_nccf, cells * 2u * n_states, d_raw, cells * 2u)) || (stage == 3 && !apart(d_raw, cells * 2u, d_out, cells * lines)))
        return ALACGPU_ERR_BAD_ARG;
    if (rows == 0 || out_frames == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    scratch_hold hold{ctx->kaldi_pitch, stream};
    int rc = ctx->kaldi_pitch.acquire(ctx, stream, (size_t)sc.bytes0, align_up(sc.bytes0 + sc.bytes0 / 4, 4096), (size_t)sc.bytes1,
                                      align_up(sc.bytes1 + sc.bytes1 / 4, 4096));
    if (rc) return rc;
    const alac_kpitch_tables tab = alac_kpitch_tables_at((const float*)d_table, phases, down_taps, n_states, up_taps);
    char* buf = (char*)ctx->kaldi_pitch.buf[0];
    float* nccf = stage == 0 ? (float*)(buf + sc.nccf) : (float*)d_nccf;
    if (front) {
        alac_kpitch_down_params q;
        q.src = (const float*)d_src;
        q.valid = (const int64_t*)d_valid;
        q.down = (float*)(buf + sc.down);
        q.sums = (double*)(buf + sc.sums);
        q.tab = tab;
        q.fr = fr;
        q.channels = channels;
        q.phases = phases;
        q.in_per_unit = in_per_unit;
        q.down_taps = down_taps;
        q.chunks = (uint32_t)chunks;
        q.stride = stride;
        q.frames = frames;
        q.n_max = n_max;
        void* kargs[] = {&q};
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_kpitch_down_kernel, dim3((uint32_t)(planes * chunks)), dim3(ALAC_KPITCH_THREADS), kargs, 0,
                                     stream));
        alac_kpitch_nccf_params n;
        n.valid = (const int64_t*)d_valid;
        n.down = q.down;
        n.sums = q.sums;
        n.nccf = nccf;
        n.tab = tab;
        n.fr = fr;
        n.channels = channels;
        n.chunks = (uint32_t)chunks;
        n.first_lag = first_lag;
        n.last_lag = last_lag;
        n.n_states = n_states;
        n.up_taps = up_taps;
        n.groups = (uint32_t)groups;
        n.frames = frames;
        n.n_max = n_max;
        n.out_frames = out_frames;
        void* nargs[] = {&n};
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_kpitch_nccf_kernel, dim3((uint32_t)(planes * groups)), dim3(ALAC_KPITCH_THREADS), nargs,
                                     alac_kpitch_nccf_lds(window, first_lag, last_lag), stream));
    }
    if (stage != 1) {
        alac_kpitch_decode_params q;
        q.nccf = decode ? nccf : nullptr;
        q.valid = (const int64_t*)d_valid;
        q.back = (uint16_t*)ctx->kaldi_pitch.buf[1];
        q.raw = stage >= 2 ? (float*)d_raw : (process ? (float*)(buf + sc.raw) : (float*)d_out);
        q.work = epilogue ? (float*)(buf + sc.work) : nullptr;
        q.out = epilogue ? (float*)d_out : nullptr;
        q.tab = tab;
        q.fr = fr;
        q.channels = channels;
        q.n_states = n_states;
        q.flags = flags;
        q.left = left_context;
        q.right = right_context;
        q.delta_window = delta_window;
        q.counts_are_frames = stage >= 2 ? 1u : 0u;
        q.frames = frames;
        q.out_frames = out_frames;
        void* kargs[] = {&q};
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_kpitch_decode_kernel, dim3((uint32_t)planes), dim3(ALAC_KPITCH_DECODE_THREADS), kargs, 0,
                                     stream));
    }
    HIP_TRY(ctx, hipGetLastError());
    return ctx->kaldi_pitch.release(ctx, stream);
}

int alacgpu_cqt_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride, uint64_t frames,
                       uint32_t hop, uint32_t n_bins, const uint32_t* lengths, const void* d_lengths, const void* d_table, int power,
                       int log_mode, float floor, void* d_out, uint64_t out_frames, void* hip_stream) {
    if (!ctx || !args_ok({{d_src, 4}, {lengths, 4}, {d_lengths, 4}, {d_table, 4}, {d_out, 4}})) return ALACGPU_ERR_BAD_ARG;
    if (n_bins < 1 || n_bins > ALAC_CQT_MAX_BINS || hop < 1 || hop > ALAC_CQT_MAX_HOP || channels == 0 || (power != 1 && power != 2))
        return ALACGPU_ERR_BAD_ARG;
    if (!(floor > 0.0f) || !std::isfinite(floor)) return ALACGPU_ERR_BAD_ARG;
    if (log_mode != ALAC_CQT_LOG_NONE && log_mode != ALAC_CQT_LOG_LN && log_mode != ALAC_CQT_LOG_10) return ALACGPU_ERR_BAD_ARG;
    if (frames < 1 || frames > src_stride || frames > (1ull << 62) || out_frames != 1u + frames / hop) return ALACGPU_ERR_BAD_ARG;
    for (uint32_t k = 0; k < n_bins; ++k)      // the lengths fall with the bin, from at most ALAC_CQT_MAX_TAPS to at least 2
        if (lengths[k] < 2u || lengths[k] > (k ? lengths[k - 1u] : ALAC_CQT_MAX_TAPS)) return ALACGPU_ERR_BAD_ARG;
    alac_cqt_params p;
    p.n0 = lengths[0];
    p.c0 = p.n0 / 2u;
    p.n_blocks = (n_bins + ALAC_CQT_BLOCK_BINS - 1u) / ALAC_CQT_BLOCK_BINS;
    uint32_t off = 0;
    for (uint32_t b = 0; b < p.n_blocks; ++b) {       // the table's layout: cqt.py's _blocks
        const uint32_t n = lengths[b * ALAC_CQT_BLOCK_BINS];
        p.blk_k[b] = (n + 1u) & ~1u;
        p.blk_off[b] = off;
        p.blk_start[b] = p.c0 - n / 2u;
        off += 32u * p.blk_k[b];
    }
    for (uint32_t b = p.n_blocks; b < ALAC_CQT_MAX_BLOCKS; ++b) p.blk_k[b] = p.blk_off[b] = p.blk_start[b] = 0u;
    const uint32_t tile = alac_cqt_tile(p.n0, hop);
    const uint64_t tiles = (out_frames + tile - 1u) / tile;
    if (tiles > 0x7FFFFFFFull || tiles * channels > 0x7FFFFFFFull || tiles * channels * rows > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    const size_t lds = sizeof(float) * (size_t)alac_cqt_lds_floats(p.n0, hop, tile);
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (lds > ALAC_CQT_LDS_DEFAULT)
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)alac_cqt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    p.src = (const float*)d_src;
    p.src_stride = src_stride;
    p.frames = frames;
    p.out = (float*)d_out;
    p.out_frames = out_frames;
    p.table = (const float*)d_table;
    p.lengths = (const uint32_t*)d_lengths;
    p.n_bins = n_bins;
    p.hop = hop;
    p.tile = tile;
    p.tiles = (uint32_t)tiles;
    p.power = (uint32_t)power;
    p.log_mode = (uint32_t)log_mode;
    p.floor = floor;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void*)alac_cqt_kernel, dim3((uint32_t)(tiles * channels * rows)), dim3(ALAC_CQT_THREADS), kargs, lds,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

int alacgpu_stft_device(alacgpu_ctx* ctx, const void* d_src, uint32_t rows, uint32_t channels, uint64_t src_stride, uint64_t frames,
                        uint32_t n_fft, uint32_t hop, const void* d_window, const void* d_table, int power, uint32_t fb_lines,
                        const uint32_t* bands, const void* d_bands, const void* d_weights, int log_mode, float floor, void* d_out,
                        uint64_t out_frames, void* hip_stream) {
    const bool fb = fb_lines != 0u;
    if (!ctx || !args_ok({{d_src, 4}, {d_window, 4}, {d_table, 8}, {bands, 4, fb}, {d_bands, 4, fb}, {d_weights, 4, fb}, {d_out, 4}}))
        return ALACGPU_ERR_BAD_ARG;
    if (!alac_stft_n_fft_ok(n_fft) || hop < 1 || hop > n_fft || channels == 0 || fb_lines > ALAC_STFT_MAX_LINES) return ALACGPU_ERR_BAD_ARG;
    if (power != ALAC_STFT_COMPLEX && power != ALAC_STFT_MAGNITUDE && power != ALAC_STFT_POWER) return ALACGPU_ERR_BAD_ARG;
    if (log_mode != ALAC_STFT_LOG_NONE && log_mode != ALAC_STFT_LOG_LN && log_mode != ALAC_STFT_LOG_10) return ALACGPU_ERR_BAD_ARG;
    if (power == ALAC_STFT_COMPLEX && (fb || log_mode != ALAC_STFT_LOG_NONE)) return ALACGPU_ERR_BAD_ARG;
    if (!(floor > 0.0f) || !std::isfinite(floor)) return ALACGPU_ERR_BAD_ARG;
    if (frames < n_fft / 2u + 1u || frames > src_stride || frames > (1ull << 62) || out_frames != 1u + frames / hop) return ALACGPU_ERR_BAD_ARG;
    const uint32_t n_bins = n_fft / 2u + 1u;
    uint64_t packed = 0;
    for (uint32_t m = 0; m < fb_lines; ++m) {     // a band lies in 0 .. n_bins, its weights behind the line's before
        const uint32_t first = bands[3u * m], count = bands[3u * m + 1u];
        if (first > n_bins || count > n_bins - first || bands[3u * m + 2u] != packed) return ALACGPU_ERR_BAD_ARG;
        packed += count;
    }
    const uint32_t lines = alac_stft_lines(n_fft, power, fb_lines);
    const uint32_t tile = alac_stft_tile(n_fft, lines, fb);
    const uint64_t tiles = (out_frames + tile - 1u) / tile;
    if (tiles > 0x7FFFFFFFull || tiles * channels > 0x7FFFFFFFull || tiles * channels * rows > 0x7FFFFFFFull) return ALACGPU_ERR_BAD_ARG;
    const size_t lds = alac_stft_lds_bytes(n_fft, lines, fb, tile);
    if (lds > ALAC_STFT_LDS_MAX) return ALACGPU_ERR_BAD_ARG;      // (no shape within the limits above is)
    if (rows == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const void* const kernel = alac_stft_kernel_of(n_fft);
    if (lds > ALAC_STFT_LDS_DEFAULT) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    alac_stft_params p;
    p.src = (const float*)d_src;
    p.src_stride = src_stride;
    p.frames = frames;
    p.out = (float*)d_out;
    p.out_frames = out_frames;
    p.window = (const float*)d_window;
    p.table = (const float2*)d_table;
    p.bands = (const uint32_t*)d_bands;
    p.weights = (const float*)d_weights;
    p.hop = hop;
    p.lines = lines;
    p.fb_lines = fb_lines;
    p.tile = tile;
    p.tiles = (uint32_t)tiles;
    p.power = (uint32_t)power;
    p.log_mode = (uint32_t)log_mode;
    p.floor = floor;
    void* kargs[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(kernel, dim3((uint32_t)(tiles * channels * rows)), dim3(alac_fft_threads(n_fft)), kargs, lds,
                                 (hipStream_t)hip_stream));
    HIP_TRY(ctx, hipGetLastError());
    return ALACGPU_OK;
}

size_t alacgpu_encode_max_packet_bytes(uint32_t frames, int sample_size, int channels) {
    // an escape packet with its sample count: header 23 + 32 bits, the raw samples, the END tag
    const uint64_t bits = 23u + 32u + (uint64_t)frames * (uint64_t)(channels < 1 ? 1 : channels) * (uint64_t)(sample_size < 0 ? 0 : sample_size) + 3u;
    return (size_t)align_up((bits + 7) / 8, 16);
}

int alacgpu_encode_device(alacgpu_ctx* ctx, const void* d_pcm, uint64_t src_elems, uint32_t channels, int layout, int dtype,
                          uint64_t plane_stride, const void* d_src_first, const void* d_src_frames, const void* d_cfg_idx,
                          uint32_t n_packets, void* d_packets, uint64_t slot_bytes, void* d_sizes, void* d_status,
                          void* hip_stream) {
    if (!ctx || !args_ok({{d_pcm, 4}, {d_src_first, 8}, {d_src_frames, 4}, {d_cfg_idx, 2}, {d_packets, 16}, {d_sizes, 4}, {d_status, 4}}))
        return ALACGPU_ERR_BAD_ARG;
    if (!pcm_view_ok(d_pcm, channels, layout, dtype, plane_stride) || (slot_bytes & 15u) != 0) return ALACGPU_ERR_BAD_ARG;
    for (uint32_t i = 0; i < ctx->n_cfgs; i++) {
        const alacgpu_cfg& c = ctx->h_cfgs[i];
        if (c.num_channels != channels) return ALACGPU_ERR_BAD_ARG;
        const uint32_t frames = std::min(c.max_samples_per_frame, MAX_FRAME);
        if (slot_bytes < alacgpu_encode_max_packet_bytes(frames, c.sample_size, (int)channels)) return ALACGPU_ERR_BAD_ARG;
    }
    if (n_packets == 0) return ALACGPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    // a round: up to 16 workgroups per CU, one packet and one workspace slot each
    int n_cu = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const uint32_t round = std::min<uint32_t>(n_packets, (uint32_t)std::max(n_cu, 1) * 16u);
    const uint32_t frames = smax(ctx);
    const size_t items = (size_t)round * alac_enc_items(frames);
    const size_t code_bytes = sizeof(uint64_t) * items, pos_bytes = sizeof(uint32_t) * (items + round);
    scratch_hold hold{ctx->enc, stream};
    int rc = ctx->enc.acquire(ctx, stream, code_bytes, code_bytes, pos_bytes, pos_bytes);
    if (rc) return rc;
    alac_encode_params p;
    p.pcm = d_pcm;
    p.src_elems = src_elems;
    p.plane_stride = layout == ALACGPU_DST_PLANAR ? plane_stride : 0;
    p.channels = channels;
    p.layout = (uint32_t)layout;
    p.dtype = (uint32_t)dtype;
    p.n_packets = n_packets;
    p.src_first = (const uint64_t*)d_src_first;
    p.src_frames = (const uint32_t*)d_src_frames;
    p.cfg_idx = (const uint16_t*)d_cfg_idx;
    p.cfgs = ctx->d_cfgs;
    p.n_cfgs = ctx->n_cfgs;
    p.smax = frames;
    p.packets = (uint8_t*)d_packets;
    p.slot_bytes = slot_bytes;
    p.sizes = (uint32_t*)d_sizes;
    p.status = (int32_t*)d_status;
    p.ws_code = (uint64_t*)ctx->enc.buf[0];
    p.ws_pos = (uint32_t*)ctx->enc.buf[1];
    for (uint32_t first = 0; first < n_packets; first += round) {
        p.first_packet = first;
        alac_encode_params args = p;
        void* kargs[] = {&args};
        const dim3 grid(std::min(round, n_packets - first)), block(ALAC_ENC_THREADS);
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_encode_analyse_kernel, grid, block, kargs, 0, stream));
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_encode_codes_kernel, grid, block, kargs, 0, stream));
        HIP_TRY(ctx, hipLaunchKernel((const void*)alac_encode_emit_kernel, grid, block, kargs, 0, stream));
    }
    HIP_TRY(ctx, hipGetLastError());
    return ctx->enc.release(ctx, stream);
}

}  // extern "C"
