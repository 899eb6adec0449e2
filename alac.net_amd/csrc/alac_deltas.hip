// alac_deltas.hip -- Kaldi's add-deltas behind the features in one launch (alacgpu_deltas_device; alac.net_amd/deltas.py states
// the mathematics and the float32 order).  The work is memory: one read of the input, order + 1 writes.  A workgroup of four
// waves takes a tile of 64 consecutive frames of four lines, one line per wave, so the grid goes by elements, not by rows:
// [64, 1, 13, 198] is 832 workgroups.  A wave loads its line's tile with a halo of order * window frames on each side into
// LDS, the index clamped into 0 .. len - 1 WHILE LOADING -- the clamp is into the original features for every order, and
// nothing outside [0, len) of a line is read for a delta -- then lane t produces every order of frame t0 + t: one chain of
// fused multiply-adds per order in ascending j over 2 k W + 1 neighbouring LDS words, which neighbouring lanes read without a
// bank conflict.  Loads and stores are coalesced along t, 256 bytes per wave.  A frame at or behind len, and a row without a
// length, gets its static block copied (read where it is) and zeros in every delta block.  Every element of `out` has one
// writer; no atomics.  Compiled without contraction: every fused multiply-add is the one written.
#include "alac_deltas.h"

__global__ __launch_bounds__(ALAC_DELTAS_THREADS) void alac_deltas_kernel(alac_deltas_params p) {
    __shared__ float xs[ALAC_DELTAS_LINES][ALAC_DELTAS_TILE + 2u * ALAC_DELTAS_MAX_HALO];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)(blockIdx.x % p.tiles) * ALAC_DELTAS_TILE;
    const uint64_t line = (uint64_t)(blockIdx.x / p.tiles) * ALAC_DELTAS_LINES + w;
    const bool line_ok = line < p.lines;
    const uint32_t halo = p.order * p.window;
    const float* const src = p.src + (line_ok ? line : 0u) * p.src_stride;
    int64_t len = 0;
    if (line_ok) {
        len = p.lengths ? p.lengths[line / p.lines_per_row] : (int64_t)p.line_len;
        len = len < 0 ? 0 : len > (int64_t)p.line_len ? (int64_t)p.line_len : len;
    }
    if (len > 0)
        for (uint32_t i = lane; i < ALAC_DELTAS_TILE + 2u * halo; i += 64u) {
            int64_t g = (int64_t)t0 - (int64_t)halo + (int64_t)i;
            g = g < 0 ? 0 : g > len - 1 ? len - 1 : g;
            xs[w][i] = src[g];
        }
    __syncthreads();

    const uint64_t t = t0 + lane;
    if (!line_ok || t >= p.line_len) return;
    const bool signal = (int64_t)t < len;
    const uint64_t block = (uint64_t)p.n_feats * p.out_stride;                    // the elements of one order's lines of a plane
    float* out = p.out + ((line / p.n_feats) * (p.order + 1u) * p.n_feats + line % p.n_feats) * p.out_stride + t;
    *out = signal ? xs[w][halo + lane] : src[t];
    const float* scales = p.scales;
    for (uint32_t k = 1; k <= p.order; ++k) {
        const uint32_t half = k * p.window;
        const float* const x = &xs[w][halo + lane - half];
        float acc = 0.0f;
        if (signal)
            for (uint32_t j = 0; j <= 2u * half; ++j) acc = __builtin_fmaf(scales[j], x[j], acc);
        out += block;
        *out = acc;
        scales += 2u * half + 1u;
    }
}
