// alac_mix.hip -- noise at a target signal-to-noise ratio into the crops, between the waveform and its features: a reduce
// launch (the sums of the squares of every part of a row's signal and noise) and an apply launch (the gain from a row's parts,
// then y = x + g n over the same part), no atomics.  include/alacgpu.h states the arithmetic, alac_mix.h the parts and the
// order of the sums.  Every operation is one IEEE float32 operation, rounded once: this file is compiled with
// -ffp-contract=off and the products and sums go through __fmul_rn / __fadd_rn, so no multiply is fused into an add; the
// divisions are `/` and the root sqrtf, which -fhip-fp32-correctly-rounded-divide-sqrt makes the correctly rounded ones.
// src and out may be the same array: a thread writes a frame only after it has read that frame, and no other thread reads it;
// the noise never overlaps out.
#include "alac_mix.h"

#pragma clang fp contract(off)

namespace {

// min(max(valid[row], 0), frames), frames without `valid`
__device__ inline uint64_t valid_of(const int64_t* valid, uint32_t row, uint64_t frames) {
    if (!valid) return frames;
    const int64_t a = valid[row];
    return a <= 0 ? 0u : ((uint64_t)a < frames ? (uint64_t)a : frames);
}

// The frames i .. i + 3 of a plane below `end`, 0 for those at or behind it (they are not read): one 16-byte load where VEC
// and all four are below `end`, 4-byte loads otherwise
template <bool VEC>
__device__ inline void load4(const float* x, uint64_t i, uint64_t end, float (&a)[ALAC_MIX_VEC]) {
    if (VEC && i + ALAC_MIX_VEC <= end) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < ALAC_MIX_VEC; k++) a[k] = i + k < end ? x[i + k] : 0.0f;
    }
}

// The sum of the squares of the frames f0 .. end of `channels` planes in alac_mix.h's order, in every thread.  wsum: one
// float per wave in LDS; it may be used again behind the call.
template <bool VEC>
__device__ inline float part_squares(const float* plane, uint64_t stride, uint32_t channels, uint64_t f0, uint64_t end, float* wsum) {
    constexpr int WAVES = ALAC_MIX_THREADS / 64;
    float q[ALAC_MIX_VEC] = {};
    for (uint32_t c = 0; c < channels; c++) {
        const float* x = plane + (uint64_t)c * stride;
        for (uint64_t i = f0 + (uint64_t)ALAC_MIX_VEC * threadIdx.x; i < end; i += ALAC_MIX_ROUND) {
            float a[ALAC_MIX_VEC];
            load4<VEC>(x, i, end, a);
#pragma unroll
            for (uint32_t k = 0; k < ALAC_MIX_VEC; k++) q[k] = __fadd_rn(q[k], __fmul_rn(a[k], a[k]));   // (+0 for a frame behind `end`)
        }
    }
    float s = __fadd_rn(__fadd_rn(q[0], q[2]), __fadd_rn(q[1], q[3]));
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) s = __fadd_rn(s, __shfl_xor(s, h, 64));
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    float w[WAVES];
#pragma unroll
    for (int j = 0; j < WAVES; j++) w[j] = wsum[j];
#pragma unroll
    for (int h = WAVES / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int j = 0; j < h; j++) w[j] = __fadd_rn(w[j], w[j + h]);
    __syncthreads();
    return w[0];
}

// What both launches know of their workgroup's row and part
struct mix_part {
    uint32_t row;
    uint64_t f0, f1, v, vn;
    float a;
    bool live;                    // the row may get noise: a != 0 (a NaN included), v and vn not 0
    __device__ mix_part(const alac_mix_params& p) {
        row = blockIdx.x / p.parts;
        f0 = (uint64_t)(blockIdx.x % p.parts) * p.part_frames;
        f1 = f0 + p.part_frames < p.frames ? f0 + p.part_frames : p.frames;
        v = valid_of(p.valid, row, p.frames);
        vn = valid_of(p.noise_valid, row, p.frames);
        a = p.ratio[row];
        live = !(a == 0.0f) && v != 0u && vn != 0u;
    }
};

// y = x + g n over the frames f0 .. f1 of every channel below v (mixing), x itself behind v where out is not src
template <bool VEC>
__device__ inline void apply_part(const alac_mix_params& p, const mix_part& w, float g, bool mixing) {
    const uint64_t planes = (uint64_t)w.row * p.channels;
    const float* noise = p.noise + (uint64_t)w.row * p.noise_channels * p.noise_stride;
    const uint64_t last = p.out != p.src ? p.frames : w.v;
    const uint64_t end = w.f1 < last ? w.f1 : last;
    const uint64_t first = w.f0 + (uint64_t)ALAC_MIX_VEC * threadIdx.x;
    const bool tiled = mixing && w.vn < w.v;          // the noise is repeated: frame i of the signal gets frame i mod vn
    uint64_t m0 = 0, step = 0;
    if (tiled) {
        m0 = first % w.vn;                                // once per thread; then advanced a round at a time
        step = ALAC_MIX_ROUND % w.vn;
    }
    for (uint32_t c = 0; c < p.channels; c++) {
        const float* x = p.src + (planes + c) * p.stride;
        float* y = p.out + (planes + c) * p.stride;
        const float* n = noise + (uint64_t)(p.noise_channels == 1u ? 0u : c) * p.noise_stride;
        uint64_t m = m0;
        for (uint64_t i = first; i < end; i += ALAC_MIX_ROUND) {
            float a[ALAC_MIX_VEC];
            load4<VEC>(x, i, end, a);
            if (mixing && i < w.v) {
                float b[ALAC_MIX_VEC];
                if (!tiled) {                             // vn >= v: frame i of the noise, read below v only
                    if (p.noise_vec) load4<true>(n, i, w.v, b);
                    else load4<false>(n, i, w.v, b);
                } else {
                    uint64_t mk = m;
#pragma unroll
                    for (uint32_t k = 0; k < ALAC_MIX_VEC; k++) {
                        b[k] = i + k < w.v ? n[mk] : 0.0f;
                        mk = mk + 1u == w.vn ? 0u : mk + 1u;
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < ALAC_MIX_VEC; k++)
                    if (i + k < w.v) a[k] = __fadd_rn(a[k], __fmul_rn(g, b[k]));
            }
            if (VEC && i + ALAC_MIX_VEC <= end) {
                *reinterpret_cast<float4*>(y + i) = make_float4(a[0], a[1], a[2], a[3]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < ALAC_MIX_VEC; k++)
                    if (i + k < end) y[i + k] = a[k];
            }
            m += step;
            if (m >= w.vn) m -= w.vn;
        }
    }
}

}  // namespace

// The sums of the squares of part blockIdx.x % parts of row blockIdx.x / parts, of the signal below v and of the noise below
// vn, into sums[blockIdx.x]; a row that gets no noise whatever its sums (a == 0, v == 0 or vn == 0) reads neither
__global__ __launch_bounds__(ALAC_MIX_THREADS) void alac_mix_reduce_kernel(alac_mix_params p) {
    __shared__ float wsum[ALAC_MIX_THREADS / 64];
    const mix_part w(p);
    float sx = 0.0f, sn = 0.0f;
    if (w.live) {                                         // (the row's: every thread takes these branches or none)
        const uint64_t ex = w.f1 < w.v ? w.f1 : w.v, en = w.f1 < w.vn ? w.f1 : w.vn;
        if (w.f0 < ex) {
            const float* x = p.src + (uint64_t)w.row * p.channels * p.stride;
            sx = p.vec ? part_squares<true>(x, p.stride, p.channels, w.f0, ex, wsum) : part_squares<false>(x, p.stride, p.channels, w.f0, ex, wsum);
        }
        if (w.f0 < en) {
            const float* n = p.noise + (uint64_t)w.row * p.noise_channels * p.noise_stride;
            sn = p.noise_vec ? part_squares<true>(n, p.noise_stride, p.noise_channels, w.f0, en, wsum)
                             : part_squares<false>(n, p.noise_stride, p.noise_channels, w.f0, en, wsum);
        }
    }
    if (threadIdx.x == 0) {
        p.sums[2u * (uint64_t)blockIdx.x] = sx;
        p.sums[2u * (uint64_t)blockIdx.x + 1u] = sn;
    }
}

// g from the row's sums, the parts in ascending order, then the workgroup's part of y.  g == 0: a copy where out is not src,
// nothing in place; the noise is not read.
__global__ __launch_bounds__(ALAC_MIX_THREADS) void alac_mix_apply_kernel(alac_mix_params p) {
    const mix_part w(p);
    float g = 0.0f;
    if (w.live) {
        const float* s = p.sums + 2u * (uint64_t)w.row * p.parts;
        float sx = 0.0f, sn = 0.0f;
        for (uint32_t k = 0; k < p.parts; k++) {          // (the same addresses in every thread)
            sx = __fadd_rn(sx, s[2u * k]);
            sn = __fadd_rn(sn, s[2u * k + 1u]);
        }
        const float ps = sx / (float)((uint64_t)p.channels * w.v);
        const float pn = sn / (float)((uint64_t)p.noise_channels * w.vn);
        if (!(pn == 0.0f)) g = __fmul_rn(w.a, sqrtf(ps / pn));
    }
    const bool mixing = !(g == 0.0f);
    if (!mixing && p.out == p.src) return;
    if (p.vec) apply_part<true>(p, w, g, mixing);
    else apply_part<false>(p, w, g, mixing);
}
