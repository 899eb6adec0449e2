// alac_normalize.h -- the launch parameters, the thresholds and the grids of the two normalisations behind the crops and the
// features (alac_normalize.hip), shared with the C ABI (alacgpu_stages.hip).  The data of both is float32
// [rows, lines_per_row, line_stride] of which the first line_len elements of a line are data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- mean and variance per line ---------------------------------------------------------------------------------------------------
// Three mappings of lines to waves, chosen from line_len alone:
//   line_len <= ALAC_NORM_WAVE_MAX   a wave per line, ALAC_NORM_WAVE_LINES lines per workgroup; lane j holds the elements
//                                    j, j + 64, j + 128, j + 192 in registers between the passes
//   line_len <= ALAC_NORM_LDS_MAX    a workgroup of ALAC_NORM_LINE_THREADS threads per line; the line stays in LDS (32 KiB at
//                                    the threshold, two workgroups per CU) between the passes
//   above                            the same workgroup; the passes read the line again from memory (it is L2's by then)
// The order of the float32 sums, which the twin in alac.net_amd/normalize.py follows: with P = 64 partial sums in the first
// mapping and P = ALAC_NORM_LINE_THREADS in the others, partial j is ((0 + t[j]) + t[j + P]) + t[j + 2 P] ... in ascending
// index over the valid elements; the 64 partials of a wave are then added as a tree of halves, q[j] = q[j] + q[j + h] for
// h = 32, 16, 8, 4, 2, 1, and the 16 wave sums of a workgroup by the same tree, h = 8, 4, 2, 1.
constexpr int ALAC_NORM_WAVE_THREADS = 256;
constexpr uint32_t ALAC_NORM_WAVE_LINES = 4u;
constexpr uint32_t ALAC_NORM_WAVE_MAX = 256u;
constexpr int ALAC_NORM_LINE_THREADS = 1024;
constexpr uint32_t ALAC_NORM_LDS_MAX = 8192u;

struct alac_meanvar_params {
    const float* src;             // [lines, line_stride]
    float* out;                   // the same layout; may be src
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), line_len), null: line_len
    uint64_t lines;               // rows * lines_per_row
    uint32_t lines_per_row;
    uint64_t line_stride, line_len;
    uint32_t centre, scale;       // 0 / 1, not both 0
    float eps;
};

// The workgroups of a mean-variance launch
__host__ __device__ inline uint64_t alac_meanvar_grid(uint64_t lines, uint64_t line_len) {
    return line_len <= ALAC_NORM_WAVE_MAX ? (lines + ALAC_NORM_WAVE_LINES - 1u) / ALAC_NORM_WAVE_LINES : lines;
}

__global__ void alac_meanvar_wave_kernel(alac_meanvar_params p);
__global__ void alac_meanvar_lds_kernel(alac_meanvar_params p);
__global__ void alac_meanvar_mem_kernel(alac_meanvar_params p);

// ---- the clamp relative to the maximum of a row -----------------------------------------------------------------------------------
// A row is the lines_per_row * line_len elements of its lines, counted line after line.  A workgroup of ALAC_TOP_THREADS
// takes one part of a row: ALAC_TOP_PART consecutive elements, or the smallest multiple of that which keeps a row within
// ALAC_TOP_MAX_PARTS parts (rows of 2^22 elements and more).
constexpr int ALAC_TOP_THREADS = 256;
constexpr uint32_t ALAC_TOP_PART = 4096u;
constexpr uint32_t ALAC_TOP_MAX_PARTS = 1024u;

__host__ __device__ inline uint64_t alac_top_part_elems(uint64_t row_elems) {
    const uint64_t least = (row_elems + ALAC_TOP_PART - 1u) / ALAC_TOP_PART;                  // parts of ALAC_TOP_PART
    const uint64_t k = (least + ALAC_TOP_MAX_PARTS - 1u) / ALAC_TOP_MAX_PARTS;
    return (uint64_t)ALAC_TOP_PART * (k ? k : 1u);
}
__host__ __device__ inline uint32_t alac_top_parts(uint64_t row_elems) {
    const uint64_t part = alac_top_part_elems(row_elems);
    return (uint32_t)((row_elems + part - 1u) / part);
}

struct alac_top_params {
    const float* src;             // [rows, lines_per_row, line_stride]
    float* out;                   // the same layout; may be src
    float* maxima;                // [rows, parts]: written by the reduce launch, read by the apply launch
    uint32_t lines_per_row;
    uint64_t line_stride, line_len;
    uint64_t row_elems;           // lines_per_row * line_len
    uint64_t part_elems;          // alac_top_part_elems(row_elems)
    uint32_t parts;               // alac_top_parts(row_elems): blockIdx.x = row * parts + part
    float top, scale, offset;
    uint32_t relative;
};

__global__ void alac_top_reduce_kernel(alac_top_params p);
__global__ void alac_top_apply_kernel(alac_top_params p);
