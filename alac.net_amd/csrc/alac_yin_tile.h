// alac_yin_tile.h -- the tile body of the YIN kernels (alac_yin.hip, alac_pyin.hip): where a workgroup's tile lies, its samples
// into LDS, step 1 (the difference functions) and step 2 (the scan that makes d' of them).  alac_yin.h states the tiling,
// alac.net_amd/yin.py every operation in order.  Every sum, difference and product goes through __fadd_rn / __fsub_rn / __fmul_rn /
// __fmaf_rn and the division is compiled as the correctly rounded one by both files (-ffp-contract=off,
// -fhip-fp32-correctly-rounded-divide-sqrt): the header has no expression whose bits depend on who includes it.
#pragma once
#include "alac_yin.h"

#pragma clang fp contract(off)

namespace {

// What one lane of a wave wrote to LDS, seen by the others of that wave
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool VEC>
__device__ inline void load4(const float* q, float* o) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = q[k];
    }
}

// The tile of a workgroup: its plane, its first frame, the row's valid samples and frame count, the frames of the tile that exist
struct yin_tile_at {
    uint32_t plane, nf;
    uint64_t t0, v, count;
};

__device__ inline yin_tile_at yin_tile_where(const alac_yin_params& p) {
    yin_tile_at at;
    at.plane = blockIdx.x / p.tiles;
    const uint32_t tile = blockIdx.x - at.plane * p.tiles, row = at.plane / p.channels;
    const uint64_t n = p.frames;
    at.v = n;
    if (p.valid) {
        const int64_t a = p.valid[row];
        at.v = a <= 0 ? 0u : ((uint64_t)a < n ? (uint64_t)a : n);
    }
    at.count = p.align ? (at.v < p.align ? 0u : 1u + (at.v - p.align) / p.hop) : at.v / p.hop + 1u;
    if (at.count > p.out_frames) at.count = p.out_frames;
    at.t0 = (uint64_t)tile * p.tile;
    at.nf = at.t0 >= at.count ? 0u : (at.count - at.t0 < p.tile ? (uint32_t)(at.count - at.t0) : p.tile);
    return at;
}

// The tile's samples into lds and step 1 by the whole workgroup (at.nf > 0): returns the difference functions, [nf, tau_max + 1]
// behind the samples, ready for a wave per frame
template <bool VEC>
__device__ inline float* yin_tile_difference(const alac_yin_params& p, float* lds, const yin_tile_at& at) {
    const uint32_t tid = threadIdx.x, nf = at.nf;
    // the tile's samples, zeros outside [0, v): nothing at or behind v is read
    const float* x = p.src + (uint64_t)at.plane * p.stride;
    const int64_t g0 = p.first + (int64_t)(at.t0 * p.hop);
    for (uint32_t i = tid; i < p.samples; i += ALAC_YIN_THREADS) {
        const int64_t g = g0 + (int64_t)i;
        lds[i] = g >= 0 && (uint64_t)g < at.v ? x[g] : 0.0f;
    }
    __syncthreads();
    // step 1
    const uint32_t lags = p.tau_max + 1u, groups = (lags + ALAC_YIN_LAGS - 1u) / ALAC_YIN_LAGS, win = p.win;
    float* dd = lds + p.samples;
    for (uint32_t item = tid; item < nf * groups; item += ALAC_YIN_THREADS) {
        const uint32_t f = item / groups, tau0 = (item - f * groups) * ALAC_YIN_LAGS;
        const float* xa = lds + (size_t)f * p.hop;
        const float* xb = xa + tau0;
        float acc[ALAC_YIN_LAGS] = {0.0f, 0.0f, 0.0f, 0.0f};
        float w[8];
        load4<VEC>(xb, w);
        for (uint32_t j = 0; j < win; j += 4u) {
            float a[4];
            load4<VEC>(xa + j, a);
            load4<VEC>(xb + j + 4u, w + 4);
#pragma unroll
            for (int jj = 0; jj < 4; jj++)
#pragma unroll
                for (int r = 0; r < (int)ALAC_YIN_LAGS; r++) {
                    const float e = __fsub_rn(a[jj], w[jj + r]);
                    acc[r] = __fmaf_rn(e, e, acc[r]);
                }
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = w[k + 4];
        }
#pragma unroll
        for (int r = 0; r < (int)ALAC_YIN_LAGS; r++)
            if (tau0 + r < lags) dd[(size_t)f * lags + tau0 + r] = acc[r];
    }
    __syncthreads();
    return dd;
}

// Step 2 of one frame by one wave: d [tau_max + 1] in LDS becomes d' in place, seen by the whole wave on return; returns
// c[tau_max] (uniform over the wave; 0: silence, d' is 1 everywhere)
__device__ inline float yin_dprime(uint32_t tau_max, float* d, uint32_t lane) {
    float carry = 0.0f;
    for (uint32_t base = 1u; base <= tau_max; base += 64u) {
        const uint32_t tau = base + lane;
        const float dv = tau <= tau_max ? d[tau] : 0.0f;
        float v = dv;
#pragma unroll
        for (uint32_t h = 1u; h < 64u; h <<= 1) {
            const float o = __shfl_up(v, h, 64);
            if (lane >= h) v = __fadd_rn(v, o);
        }
        const float c = __fadd_rn(carry, v);
        carry = __shfl(c, 63, 64);
        if (tau <= tau_max) d[tau] = c != 0.0f ? __fmul_rn(dv, (float)tau) / c : 1.0f;
    }
    if (lane == 0u) d[0] = 1.0f;
    wave_sync();
    return carry;
}

}  // namespace
