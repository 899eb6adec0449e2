// alac_biquad.hip -- a cascade of biquad sections and a gain per row on the waveform, between the noise mix and the features:
// one launch, no atomics, no scratch.  include/alacgpu.h states the arithmetic, alac_biquad.h the blocking, alac.net_amd/biquad.py
// every operation in order.  The recurrences are float64: every operation is one IEEE float64 operation, rounded once -- this
// file is compiled with -ffp-contract=off and the products and sums go through __dmul_rn / __dadd_rn / __dsub_rn, so no multiply
// is fused into an add and the twin needs no float64 FMA.  src and out may be the same array: a lane stores the frames it
// loaded itself, and no other lane reads them.
#include "alac_biquad_tile.h"

using namespace alac_biquad_tile;

namespace {

template <bool VEC>
__device__ inline void biquad_plane(const alac_biquad_params& p, const float* x, float* y, uint64_t v, double g, const double* tab,
                                    state* hist, state* wtot, state* carry) {
    const uint32_t tid = threadIdx.x;
    const uint32_t S = p.sections;
    uint32_t par = 0;                                     // the tile's parity: which half of hist and carry it writes
    for (uint64_t t0 = 0; t0 < v; t0 += ALAC_BIQUAD_TILE, par ^= 1u) {
        const uint64_t n0 = t0 + (uint64_t)CHUNK * tid;
        double u[CHUNK];
        const bool whole = load_chunk<VEC>(x, n0, v, u);
        run_sections(u, S, t0, par, tab, hist, wtot, carry);
        float r[CHUNK];
#pragma unroll
        for (uint32_t j = 0; j < CHUNK; j++) {
            float a = (float)mul(g, u[j]);
            if (p.clamp) a = a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);          // (a NaN stays one)
            r[j] = a;
        }
        if (whole) {
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j += 4u) *reinterpret_cast<float4*>(y + n0 + j) = make_float4(r[j], r[j + 1], r[j + 2], r[j + 3]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j++)
                if (n0 + j < v) y[n0 + j] = r[j];
        }
    }
}

}  // namespace

// One (row, channel) a workgroup.  A row with v == 0, and a row whose sections are all (1, 0, 0, 0, 0) with a gain of 1 and no
// clamp, is neither read nor written.
__global__ __launch_bounds__(ALAC_BIQUAD_THREADS) void alac_biquad_kernel(alac_biquad_params p) {
    __shared__ double tab[ALAC_BIQUAD_MAX_SECTIONS * ALAC_BIQUAD_TAB];
    __shared__ state hist[2 * ALAC_BIQUAD_THREADS];
    __shared__ state wtot[2 * WAVES];
    __shared__ state carry[2 * ALAC_BIQUAD_MAX_SECTIONS];
    const uint32_t row = blockIdx.x / p.channels;
    uint64_t v = p.frames;
    if (p.valid) {
        const int64_t a = p.valid[row];
        v = a <= 0 ? 0u : ((uint64_t)a < p.frames ? (uint64_t)a : p.frames);
    }
    if (v == 0u) return;                                  // (the row's: every lane returns or none)
    const double* const q = p.coeffs + (uint64_t)row * p.sections * 5u;
    const double g = p.gain ? p.gain[row] : 1.0;
    bool identity = g == 1.0 && !p.clamp;
    for (uint32_t k = 0; k < p.sections; k++)
        identity = identity && q[5u * k] == 1.0 && q[5u * k + 1u] == 0.0 && q[5u * k + 2u] == 0.0 && q[5u * k + 3u] == 0.0 &&
                   q[5u * k + 4u] == 0.0;
    if (identity) return;
    if (threadIdx.x < p.sections) make_table(q + 5u * threadIdx.x, tab + threadIdx.x * ALAC_BIQUAD_TAB);
    __syncthreads();
    const float* const x = p.src + (uint64_t)blockIdx.x * p.stride;
    float* const y = p.out + (uint64_t)blockIdx.x * p.stride;
    if (p.vec) biquad_plane<true>(p, x, y, v, g, tab, hist, wtot, carry);
    else biquad_plane<false>(p, x, y, v, g, tab, hist, wtot, carry);
}
