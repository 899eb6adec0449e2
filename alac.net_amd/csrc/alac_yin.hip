// alac_yin.hip -- the YIN pitch estimator behind the crops (de Cheveigne and Kawahara 2002, steps 1 to 5), one launch.
// include/alacgpu.h states the mathematics, alac_yin.h the tiling, alac.net_amd/yin.py every operation in order.  All float32,
// one IEEE operation at a time but for the fused multiply-adds written out: this file is compiled with -ffp-contract=off and
// -fhip-fp32-correctly-rounded-divide-sqrt, and sums, differences and products go through __fadd_rn / __fsub_rn / __fmul_rn.
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

// Steps 2 to 5 of one frame by one wave: d [tau_max + 1] in LDS becomes d' in place; lane 0 writes the frame's two values
__device__ inline void yin_frame(const alac_yin_params& p, float* d, uint32_t lane, float* f0_out, float* ap_out) {
    const uint32_t tau_max = p.tau_max, last = tau_max - 1u;
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
    float f0 = 0.0f, ap = 1.0f;
    if (carry != 0.0f) {                                           // (c[tau_max]; uniform over the wave)
        uint32_t tau = 0u;
        for (uint32_t base = p.tau_min; base <= last; base += 64u) {
            const uint32_t t = base + lane;
            const unsigned long long hit = __ballot(t <= last && d[t] < p.threshold);
            if (hit) {
                tau = base + (uint32_t)__builtin_ctzll(hit);
                break;
            }
        }
        if (tau) {
            while (tau + 1u <= last && d[tau + 1u] < d[tau]) tau++;
        } else {                                                   // the first argmin, a NaN as +infinity
            float best = __builtin_inff();
            uint32_t at = 0xFFFFFFFFu;
            for (uint32_t t = p.tau_min + lane; t <= last; t += 64u) {
                const float q = d[t];
                const float key = q != q ? __builtin_inff() : q;
                if (key < best || at == 0xFFFFFFFFu) best = key, at = t;
            }
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) {
                const float ob = __shfl_xor(best, h, 64);
                const uint32_t oa = (uint32_t)__shfl_xor((int)at, h, 64);
                if (ob < best || (ob == best && oa < at)) best = ob, at = oa;
            }
            tau = at;
        }
        const float a = d[tau - 1u], b = d[tau], c = d[tau + 1u];
        const float n = __fsub_rn(a, c), q = __fadd_rn(__fsub_rn(a, __fmul_rn(2.0f, b)), c);
        const float shift = (b <= a && b <= c && q > 0.0f) ? __fmul_rn(0.5f, n) / q : 0.0f;
        f0 = p.rate / __fadd_rn((float)tau, shift);
        ap = b;
    }
    if (lane == 0u) *f0_out = f0, *ap_out = ap;
}

template <bool VEC>
__device__ inline void yin_tile(const alac_yin_params& p, float* lds) {
    const uint32_t plane = blockIdx.x / p.tiles, tile = blockIdx.x - plane * p.tiles;
    const uint32_t row = plane / p.channels, tid = threadIdx.x;
    const uint64_t n = p.frames;
    uint64_t v = n;
    if (p.valid) {
        const int64_t a = p.valid[row];
        v = a <= 0 ? 0u : ((uint64_t)a < n ? (uint64_t)a : n);
    }
    uint64_t count = p.align ? (v < p.align ? 0u : 1u + (v - p.align) / p.hop) : v / p.hop + 1u;
    if (count > p.out_frames) count = p.out_frames;
    const uint64_t t0 = (uint64_t)tile * p.tile;
    float* f0_line = p.out + (uint64_t)plane * 2u * p.out_frames;
    float* ap_line = f0_line + p.out_frames;
    // the frames of the tile at and behind the row's count: zeros
    if (tid < p.tile) {
        const uint64_t t = t0 + tid;
        if (t >= count && t < p.out_frames) f0_line[t] = 0.0f, ap_line[t] = 0.0f;
    }
    if (t0 >= count) return;                                       // (the whole workgroup, before any load)
    const uint32_t nf = count - t0 < p.tile ? (uint32_t)(count - t0) : p.tile;
    // the tile's samples, zeros outside [0, v): nothing at or behind v is read
    const float* x = p.src + (uint64_t)plane * p.stride;
    const int64_t g0 = p.first + (int64_t)(t0 * p.hop);
    for (uint32_t i = tid; i < p.samples; i += ALAC_YIN_THREADS) {
        const int64_t g = g0 + (int64_t)i;
        lds[i] = g >= 0 && (uint64_t)g < v ? x[g] : 0.0f;
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
    // steps 2 to 5: a wave per frame
    const uint32_t lane = tid & 63u;
    for (uint32_t f = tid >> 6; f < nf; f += ALAC_YIN_THREADS / 64)
        yin_frame(p, dd + (size_t)f * lags, lane, f0_line + t0 + f, ap_line + t0 + f);
}

}  // namespace

__global__ __launch_bounds__(ALAC_YIN_THREADS) void alac_yin_kernel(alac_yin_params p) {
    extern __shared__ __align__(16) float yin_lds[];
    yin_tile<false>(p, yin_lds);
}

// hop % 4 == 0: every frame starts on a 16-byte boundary of the LDS image
__global__ __launch_bounds__(ALAC_YIN_THREADS) void alac_yin_kernel_vec(alac_yin_params p) {
    extern __shared__ __align__(16) float yin_lds[];
    yin_tile<true>(p, yin_lds);
}
