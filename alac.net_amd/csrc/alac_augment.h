// alac_augment.h -- the launch parameters, the thresholds and the grid of SpecAugment behind the features (alac_augment.hip),
// shared with the C ABI (alacgpu_stages.hip).  The data is float32 [rows, channels, n_mels, line_stride] of which the first
// line_len elements of a line are frames; a line is one mel bin of one channel of one crop, and all lines of a row share the
// row's draws: d_warp [rows, 2] (c, c'), d_freq [rows, n_freq, 2] and d_time [rows, n_time, 2] (start, width), int32.
// alac.net_amd/augment.py states the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Two mappings of lines to threads, chosen from line_len alone; both are workgroups of ALAC_AUG_THREADS threads and one launch:
//   line_len <= ALAC_AUG_WAVE_MAX    a wave per line, ALAC_AUG_WAVE_LINES lines per workgroup.  A wave covers 256 frames in
//                                    one round of 128-bit accesses (64 lanes x 4 frames); a workgroup per line would leave
//                                    three of its four waves without a frame, and features of 2 s at a hop of 10 ms (201
//                                    frames, 5120 lines in a batch of 64) are the common case.
//   above                            a workgroup per line: a line of 3000 frames is three rounds of 128-bit accesses.
// A line that is warped is staged in LDS, its valid frames only, behind the time-mask table of its row (n_time pairs; a
// table per wave in the first mapping) -- so that every frame is read before any is written and the call may be in place.
// ALAC_AUG_LDS_MAX is the longest line that can be warped: 16384 frames are 64 KiB of the CU's 160 KiB, which still leaves
// room for two workgroups of the largest kind on a CU; Whisper's 30 s are 3000 frames, 12 KiB, and twelve workgroups.  A
// call with d_warp and a longer line is refused; masks alone stage nothing and have no limit.  With line_len at most 16384
// the products t * c of the warp's source position are below 2^28: the kernel divides in 32 bits.
constexpr int ALAC_AUG_THREADS = 256;
constexpr uint32_t ALAC_AUG_WAVE_LINES = 4u;
constexpr uint32_t ALAC_AUG_WAVE_MAX = 256u;
constexpr uint32_t ALAC_AUG_LDS_MAX = 16384u;
// The most masks of a kind a call takes: their table is in LDS next to the line (8 KiB at the limit), and a frame is held
// against every pair of it
constexpr uint32_t ALAC_AUG_MAX_MASKS = 1024u;

struct alac_augment_params {
    const float* src;             // [lines, line_stride]
    float* out;                   // the same layout; may be src
    const int64_t* valid;         // [rows] or null: tau = min(max(valid[r], 0), line_len), null: line_len
    const int32_t* warp;          // [rows, 2] or null: (c, c'); a warp only where 1 <= c, c' <= tau - 2 and c != c'
    const int32_t* freq;          // [rows, n_freq, 2]: (first bin, bins)
    const int32_t* time;          // [rows, n_time, 2]: (first frame, frames)
    uint64_t lines;               // rows * lines_per_row
    uint32_t lines_per_row;       // channels * n_mels
    uint32_t n_mels, n_freq, n_time;
    uint32_t stage;               // the floats of LDS a line has for its frames: line_len with a warp, else 0
    uint64_t line_stride, line_len;
    float fill;
};

// The lines a workgroup takes, the workgroups of a launch and the dynamic LDS of one of them
__host__ __device__ inline uint32_t alac_augment_lines_per_wg(uint64_t line_len) {
    return line_len <= ALAC_AUG_WAVE_MAX ? ALAC_AUG_WAVE_LINES : 1u;
}
__host__ __device__ inline uint64_t alac_augment_grid(uint64_t lines, uint64_t line_len) {
    const uint32_t per = alac_augment_lines_per_wg(line_len);
    return (lines + per - 1u) / per;
}
__host__ __device__ inline size_t alac_augment_lds_bytes(uint64_t line_len, uint32_t n_time, bool warp) {
    return (size_t)alac_augment_lines_per_wg(line_len) * (sizeof(int32_t) * 2u * n_time + (warp ? sizeof(float) * (size_t)line_len : 0u));
}

__global__ void alac_specaugment_wave_kernel(alac_augment_params p);
__global__ void alac_specaugment_line_kernel(alac_augment_params p);
