// alac_yin.hip -- the YIN pitch estimator behind the crops (de Cheveigne and Kawahara 2002, steps 1 to 5), one launch.
// include/alacgpu.h states the mathematics, alac_yin.h the tiling, alac.net_amd/yin.py every operation in order.  All float32,
// one IEEE operation at a time but for the fused multiply-adds written out: this file is compiled with -ffp-contract=off and
// -fhip-fp32-correctly-rounded-divide-sqrt, and sums, differences and products go through __fadd_rn / __fsub_rn / __fmul_rn.
#include "alac_yin_tile.h"

#pragma clang fp contract(off)

namespace {

// Steps 2 to 5 of one frame by one wave: d [tau_max + 1] in LDS becomes d' in place; lane 0 writes the frame's two values
__device__ inline void yin_frame(const alac_yin_params& p, float* d, uint32_t lane, float* f0_out, float* ap_out) {
    const uint32_t last = p.tau_max - 1u;
    const float carry = yin_dprime(p.tau_max, d, lane);
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
    const yin_tile_at at = yin_tile_where(p);
    const uint32_t plane = at.plane, tid = threadIdx.x, nf = at.nf;
    const uint64_t t0 = at.t0;
    float* f0_line = p.out + (uint64_t)plane * 2u * p.out_frames;
    float* ap_line = f0_line + p.out_frames;
    // the frames of the tile at and behind the row's count: zeros
    if (tid < p.tile) {
        const uint64_t t = t0 + tid;
        if (t >= at.count && t < p.out_frames) f0_line[t] = 0.0f, ap_line[t] = 0.0f;
    }
    if (nf == 0u) return;                                          // (the whole workgroup, before any load)
    const uint32_t lags = p.tau_max + 1u;
    float* dd = yin_tile_difference<VEC>(p, lds, at);
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
