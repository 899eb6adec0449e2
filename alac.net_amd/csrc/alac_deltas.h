// alac_deltas.h -- the launch parameters of the delta-feature kernel (alac_deltas.hip), shared with the C ABI
// (alacgpu_stages.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ALAC_DELTAS_THREADS = 256;
constexpr uint32_t ALAC_DELTAS_TILE = 64u;              // consecutive frames of a workgroup's tile: a wave's lanes
constexpr uint32_t ALAC_DELTAS_LINES = 4u;              // lines of a tile: a workgroup's waves
constexpr uint32_t ALAC_DELTAS_MAX_ORDER = 3u;
constexpr uint32_t ALAC_DELTAS_MAX_WINDOW = 4u;
constexpr uint32_t ALAC_DELTAS_MAX_HALO = ALAC_DELTAS_MAX_ORDER * ALAC_DELTAS_MAX_WINDOW;   // frames on each side of a tile

// The scales of order k = 1 .. order, 2 k W + 1 of them, begin at float W k (k - 1) + (k - 1) of the table; all of them:
__host__ __device__ inline uint32_t alac_deltas_scales(uint32_t order, uint32_t window) { return window * order * (order + 1u) + order; }

struct alac_deltas_params {
    const float* src;             // [lines, src_stride]; line = (row * channels + channel) * n_feats + f
    float* out;                   // [lines / n_feats, (order + 1) * n_feats, out_stride]
    const int64_t* lengths;       // [rows] or null
    const float* scales;          // [alac_deltas_scales(order, window)]
    uint64_t lines;               // rows * lines_per_row
    uint64_t src_stride, out_stride, line_len;
    uint32_t lines_per_row;       // channels * n_feats
    uint32_t n_feats;
    uint32_t order, window;
    uint32_t tiles;               // ceil(line_len / ALAC_DELTAS_TILE): blockIdx.x = group of lines * tiles + tile index
};

__global__ void alac_deltas_kernel(alac_deltas_params p);
