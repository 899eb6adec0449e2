// alac_vad.h -- the launch parameters, the thresholds and the grids of the energy VAD and of the selection of the voiced frames
// behind the features (alac_vad.hip), shared with the C ABI (alacgpu_stages.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- the decision ------------------------------------------------------------------------------------------------------------------
// A team of threads takes a row: the mean of its energy line over the valid frames in alac_normalize.h's order, the threshold,
// then a thread per frame counts the frames within frames_context that are above it.  Two teams, chosen from line_len alone:
//   line_len <= ALAC_VAD_WAVE_MAX   a wave per row (P = 64 partial sums), ALAC_VAD_WAVE_ROWS rows per workgroup of ALAC_VAD_WAVE_THREADS
//   above                           a workgroup of ALAC_VAD_LINE_THREADS threads per row (P = ALAC_VAD_LINE_THREADS)
// mean = sum / fl(v), thr = threshold + fl(scale * mean), each rounded once; with a scale of 0 the mean is not computed.
constexpr int ALAC_VAD_WAVE_THREADS = 256;
constexpr uint32_t ALAC_VAD_WAVE_ROWS = 4u;
constexpr uint32_t ALAC_VAD_WAVE_MAX = 256u;
constexpr int ALAC_VAD_LINE_THREADS = 1024;
constexpr uint32_t ALAC_VAD_MAX_CONTEXT = 64u;

struct alac_vad_params {
    const float* energy;          // the energy line of row 0; row r's is row_stride elements further
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), line_len), null: line_len
    uint8_t* mask;                // [rows, mask_stride]: the first line_len of a row are written
    uint32_t rows;
    uint64_t row_stride, line_len, mask_stride;
    float threshold, mean_scale, proportion;
    uint32_t context;
};

__host__ __device__ inline uint64_t alac_vad_grid(uint64_t rows, uint64_t line_len) {
    return line_len <= ALAC_VAD_WAVE_MAX ? (rows + ALAC_VAD_WAVE_ROWS - 1u) / ALAC_VAD_WAVE_ROWS : rows;
}

__global__ void alac_vad_wave_kernel(alac_vad_params p);
__global__ void alac_vad_line_kernel(alac_vad_params p);

// ---- the selection -----------------------------------------------------------------------------------------------------------------
// A workgroup of ALAC_SELECT_THREADS takes ALAC_SELECT_LINES consecutive lines of a row (all lines of the row when the new
// lengths are written over the old ones: no other workgroup may then read the row's length) and walks them in chunks of
// ALAC_SELECT_CHUNK frames in ascending order, a frame per thread: the exclusive count of the chunk's voiced frames from a
// ballot per wave and the wave totals in LDS, the running count carried from chunk to chunk; every line's chunk is read, then
// a barrier, then stored at the counts -- a frame only moves left, so out may be src.  [voiced, line_len) is zeroed at the end.
constexpr int ALAC_SELECT_THREADS = 1024;
constexpr uint32_t ALAC_SELECT_CHUNK = 1024u;
constexpr uint32_t ALAC_SELECT_LINES = 8u;

struct alac_select_params {
    const float* src;             // [rows, lines_per_row, line_stride]
    float* out;                   // the same layout; may be src
    const int64_t* valid;         // [rows] or null
    const uint8_t* mask;          // [rows, mask_stride]
    int64_t* new_lengths;         // [rows]; may be valid
    uint32_t lines_per_row;
    uint32_t groups;              // workgroups per row: 1, or ceil(lines_per_row / ALAC_SELECT_LINES)
    uint64_t line_stride, line_len, mask_stride;
};

__global__ void alac_select_frames_kernel(alac_select_params p);
