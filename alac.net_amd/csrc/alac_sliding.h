// alac_sliding.h -- the launch parameters, the thresholds and the grid of the sliding-window mean-variance normalisation behind
// the features (alac_sliding.hip), shared with the C ABI (alacgpu_stages.hip).  The data is float32
// [rows, lines_per_row, line_stride] of which the first line_len elements of a line are data, as in alac_normalize.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A team of threads takes a line: it computes the pivot p (the mean of the line's finite valid elements), holds d = x - p and
// the sums of d's blocks of ALAC_SLIDING_BLOCK frames (and of d * d's, with norm_vars) in LDS, and then a thread takes a frame:
// its window's head elements, whole blocks and tail elements in one chain of additions.  Two teams, chosen from line_len alone:
//   line_len <= ALAC_SLIDING_WAVE_MAX   a wave per line, ALAC_SLIDING_WAVE_LINES lines per workgroup of ALAC_SLIDING_WAVE_THREADS
//   above                               a workgroup of ALAC_SLIDING_LINE_THREADS threads per line
// A line of up to ALAC_SLIDING_LDS_MAX frames is held whole: 64 KiB of d and 2 * 2 KiB of block sums at the limit, 68 KiB of the
// 160 KiB of a gfx950 CU, so two workgroups still fit.  A longer line goes through the same LDS as a ring of ALAC_SLIDING_LDS_MAX
// frames: the team takes the frames in chunks of its size in ascending order and in front of each chunk reads from memory what
// the chunk's windows reach -- a second read of the line, behind the pivot's -- so that every frame is read before the chunk
// that writes it, and d_out may be d_src.  The ring holds a chunk and `window` + a block on both sides of it, hence
// ALAC_SLIDING_RING_WINDOW_MAX: the widest window of a line above ALAC_SLIDING_LDS_MAX.
// The order of the float32 operations, which the twin in alac.net_amd/sliding.py follows: the pivot's sum as
// alac_normalize.h's mean (P = 64 partial sums in the first team, ALAC_SLIDING_LINE_THREADS in the second; an element that is
// not finite counts as +0), p = sum / fl(v); a block's sum a tree of halves, q[j] = q[j] + q[j + h] for h = 16 .. 1, elements at
// or behind v counting as +0; a window [s, e) from zero: the elements s .. 32 j0 - 1, the blocks j0 .. j1 - 1, the elements
// 32 j1 .. e - 1, each ascending, j0 = ceil(s / 32), j1 = floor(e / 32) -- all elements ascending where j0 >= j1.
constexpr uint32_t ALAC_SLIDING_BLOCK = 32u;
constexpr int ALAC_SLIDING_WAVE_THREADS = 256;
constexpr uint32_t ALAC_SLIDING_WAVE_LINES = 4u;
constexpr uint32_t ALAC_SLIDING_WAVE_MAX = 256u;
constexpr int ALAC_SLIDING_LINE_THREADS = 1024;
constexpr uint32_t ALAC_SLIDING_LDS_MAX = 16384u;
constexpr uint32_t ALAC_SLIDING_RING_WINDOW_MAX = 7648u;
static_assert(ALAC_SLIDING_LINE_THREADS + 2u * (ALAC_SLIDING_RING_WINDOW_MAX + ALAC_SLIDING_BLOCK) <= ALAC_SLIDING_LDS_MAX,
              "a chunk, and a window and a block on both sides of it, fit the ring");
constexpr float ALAC_SLIDING_VAR_FLOOR = 1e-10f;

struct alac_sliding_params {
    const float* src;             // [lines, line_stride]
    float* out;                   // the same layout; may be src
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), line_len), null: line_len
    uint64_t lines;               // rows * lines_per_row
    uint32_t lines_per_row;
    uint64_t line_stride, line_len;
    uint32_t window, min_window;  // 1 <= min_window <= window < 2^31
    uint32_t center, norm_vars;   // 0 / 1
    uint32_t ring;                // alac_sliding_ring(line_len): the frames of LDS a team has for d
};

// The frames of d a team holds for lines of line_len: the whole line up to a power of two, at most ALAC_SLIDING_LDS_MAX
__host__ __device__ inline uint32_t alac_sliding_ring(uint64_t line_len) {
    uint32_t r = ALAC_SLIDING_BLOCK;
    while (r < ALAC_SLIDING_LDS_MAX && r < line_len) r <<= 1;
    return r;
}

// The dynamic LDS of a launch: per team d [ring] and both block sums [ring / 32]; the workgroup team's wave sums behind them
__host__ __device__ inline size_t alac_sliding_lds_bytes(uint64_t line_len) {
    const size_t team = sizeof(float) * (alac_sliding_ring(line_len) + 2u * (alac_sliding_ring(line_len) / ALAC_SLIDING_BLOCK));
    return line_len <= ALAC_SLIDING_WAVE_MAX ? ALAC_SLIDING_WAVE_LINES * team : team + sizeof(float) * (ALAC_SLIDING_LINE_THREADS / 64);
}

// The workgroups of a launch
__host__ __device__ inline uint64_t alac_sliding_grid(uint64_t lines, uint64_t line_len) {
    return line_len <= ALAC_SLIDING_WAVE_MAX ? (lines + ALAC_SLIDING_WAVE_LINES - 1u) / ALAC_SLIDING_WAVE_LINES : lines;
}

__global__ void alac_sliding_wave_kernel(alac_sliding_params p);
__global__ void alac_sliding_line_kernel(alac_sliding_params p);
