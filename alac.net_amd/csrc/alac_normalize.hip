// alac_normalize.hip -- the two normalisations between the crops or their log-mel features and a model: mean and variance per
// line over the valid elements (one launch), and the clamp relative to the maximum of a row (a reduce and an apply launch,
// no atomics).  include/alacgpu.h states the mathematics, alac_normalize.h the mappings, the order of the sums and the
// thresholds.  Every operation is one IEEE float32 operation, rounded once: this file is compiled with -ffp-contract=off and
// the products and sums that stand next to one another go through __fmul_rn / __fadd_rn, so no multiply is fused into an
// add; the divisions are `/` and the root sqrtf, which -fhip-fp32-correctly-rounded-divide-sqrt makes the correctly rounded
// ones (__fsqrt_rn is the hardware's root, good to one ulp only).  src and out may be the same array: a thread writes element i only after it has read element i for the last time,
// and no other thread reads it.
#include "alac_normalize.h"

#pragma clang fp contract(off)

namespace {

// The tree of halves over the 64 partials of a wave, q[j] = q[j] + q[j + h] for h = 32 .. 1, as a butterfly: every lane
// ends with the sum (float addition commutes, so lane j and lane j ^ h compute the same value).
__device__ inline float wave_sum(float q) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) q = __fadd_rn(q, __shfl_xor(q, h, 64));
    return q;
}

// ... and over the ALAC_NORM_LINE_THREADS / 64 wave sums of a workgroup, by the same tree, in every thread alike.  wsum:
// one float per wave in LDS; it may be used again behind the call.
__device__ inline float block_sum(float q, float* wsum) {
    constexpr int WAVES = ALAC_NORM_LINE_THREADS / 64;
    q = wave_sum(q);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = q;
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

// v of a line: min(max(valid[row], 0), line_len), line_len without `valid`
__device__ inline uint64_t valid_of(const alac_meanvar_params& p, uint64_t line) {
    if (!p.valid) return p.line_len;
    const int64_t a = p.valid[line / p.lines_per_row];
    return a <= 0 ? 0u : ((uint64_t)a < p.line_len ? (uint64_t)a : p.line_len);
}

// The element of the result from x, x - mean and s = sqrt(var + eps)
__device__ inline float meanvar_result(const alac_meanvar_params& p, float x, float d, float s) {
    if (!p.scale) return d;
    return (p.centre ? d : x) / s;
}

// A workgroup per line; LDS: the line stays in `line` between the passes, else it is read again from memory
template <bool LDS>
__device__ inline void meanvar_line(const alac_meanvar_params& p, float* line, float* wsum) {
    constexpr uint64_t T = ALAC_NORM_LINE_THREADS;
    const uint64_t l = blockIdx.x, n = p.line_len, v = valid_of(p, l), t = threadIdx.x;
    const float* x = p.src + l * p.line_stride;
    float* y = p.out + l * p.line_stride;
    if (v) {                                                      // (v is the workgroup's: every thread takes this branch or none)
        float acc = 0.0f;
        for (uint64_t i = t; i < v; i += T) {
            const float a = x[i];
            if (LDS) line[i] = a;
            acc = __fadd_rn(acc, a);
        }
        const float fv = (float)v;
        const float mean = block_sum(acc, wsum) / fv;
        float s = 1.0f;
        if (p.scale) {
            acc = 0.0f;
            for (uint64_t i = t; i < v; i += T) {
                const float d = __fsub_rn(LDS ? line[i] : x[i], mean);
                acc = __fadd_rn(acc, __fmul_rn(d, d));
            }
            s = sqrtf(__fadd_rn(block_sum(acc, wsum) / fv, p.eps));
        }
        for (uint64_t i = t; i < v; i += T) {
            const float a = LDS ? line[i] : x[i];
            y[i] = meanvar_result(p, a, __fsub_rn(a, mean), s);
        }
    }
    for (uint64_t i = v + t; i < n; i += T) y[i] = 0.0f;
}

// max(a, b) that keeps a NaN, as np.max and torch.amax do (the hardware's max returns the other operand)
__device__ inline float nan_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// nan_max over the workgroup (ALAC_TOP_THREADS), in every thread; wmax: one float per wave in LDS
__device__ inline float block_nan_max(float m, float* wmax) {
    constexpr int WAVES = ALAC_TOP_THREADS / 64;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) m = nan_max(m, __shfl_xor(m, h, 64));
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    m = wmax[0];
#pragma unroll
    for (int j = 1; j < WAVES; j++) m = nan_max(m, wmax[j]);
    return m;
}

// A thread's walk over its elements of a part: element e of the row is element i of line `line`
struct top_walk {
    uint64_t e, e1, line, i;
    __device__ top_walk(const alac_top_params& p, uint32_t part) {
        const uint64_t e0 = (uint64_t)part * p.part_elems;
        e1 = e0 + p.part_elems < p.row_elems ? e0 + p.part_elems : p.row_elems;
        e = e0 + threadIdx.x;
        line = e / p.line_len;
        i = e - line * p.line_len;
    }
    __device__ bool more() const { return e < e1; }
    __device__ uint64_t at(const alac_top_params& p) const { return line * p.line_stride + i; }
    __device__ void next(const alac_top_params& p) {
        e += ALAC_TOP_THREADS;
        i += ALAC_TOP_THREADS;
        if (i >= p.line_len) {
            const uint64_t q = i / p.line_len;
            line += q;
            i -= q * p.line_len;
        }
    }
};

}  // namespace

// A wave per line of at most ALAC_NORM_WAVE_MAX elements, the line in registers
__global__ __launch_bounds__(ALAC_NORM_WAVE_THREADS) void alac_meanvar_wave_kernel(alac_meanvar_params p) {
    constexpr uint32_t PER_LANE = ALAC_NORM_WAVE_MAX / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t l = (uint64_t)blockIdx.x * ALAC_NORM_WAVE_LINES + (threadIdx.x >> 6);
    if (l >= p.lines) return;                                     // (no barrier in this kernel)
    const uint64_t n = p.line_len, v = valid_of(p, l);
    const float* x = p.src + l * p.line_stride;
    float* y = p.out + l * p.line_stride;
    float a[PER_LANE], r[PER_LANE] = {};
    float acc = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < PER_LANE; k++) {
        const uint64_t i = lane + 64u * k;
        a[k] = i < v ? x[i] : 0.0f;
        acc = __fadd_rn(acc, a[k]);
    }
    if (v) {                                                      // (v is the wave's)
        const float fv = (float)v;
        const float mean = wave_sum(acc) / fv;
        float s = 1.0f;
        acc = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < PER_LANE; k++) {
            r[k] = __fsub_rn(a[k], mean);
            acc = __fadd_rn(acc, lane + 64u * k < v ? __fmul_rn(r[k], r[k]) : 0.0f);
        }
        if (p.scale) s = sqrtf(__fadd_rn(wave_sum(acc) / fv, p.eps));
#pragma unroll
        for (uint32_t k = 0; k < PER_LANE; k++) r[k] = meanvar_result(p, a[k], r[k], s);
    }
#pragma unroll
    for (uint32_t k = 0; k < PER_LANE; k++) {
        const uint64_t i = lane + 64u * k;
        if (i < n) y[i] = i < v ? r[k] : 0.0f;
    }
}

__global__ __launch_bounds__(ALAC_NORM_LINE_THREADS) void alac_meanvar_lds_kernel(alac_meanvar_params p) {
    __shared__ float line[ALAC_NORM_LDS_MAX];
    __shared__ float wsum[ALAC_NORM_LINE_THREADS / 64];
    meanvar_line<true>(p, line, wsum);
}

__global__ __launch_bounds__(ALAC_NORM_LINE_THREADS) void alac_meanvar_mem_kernel(alac_meanvar_params p) {
    __shared__ float wsum[ALAC_NORM_LINE_THREADS / 64];
    meanvar_line<false>(p, nullptr, wsum);
}

// The maximum of part blockIdx.x % parts of row blockIdx.x / parts into maxima[blockIdx.x], NaN where the part holds one
__global__ __launch_bounds__(ALAC_TOP_THREADS) void alac_top_reduce_kernel(alac_top_params p) {
    __shared__ float wmax[ALAC_TOP_THREADS / 64];
    const uint32_t row = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
    const float* x = p.src + (uint64_t)row * p.lines_per_row * p.line_stride;
    float m = -INFINITY;
    bool nan = false;
    for (top_walk w(p, part); w.more(); w.next(p)) {
        const float a = x[w.at(p)];
        nan |= a != a;
        m = fmaxf(m, a);
    }
    m = block_nan_max(nan ? NAN : m, wmax);
    if (threadIdx.x == 0) p.maxima[blockIdx.x] = m;
}

// mx from the row's maxima, then y = scale * (max(x, mx - top) [- mx]) + offset over the same part
__global__ __launch_bounds__(ALAC_TOP_THREADS) void alac_top_apply_kernel(alac_top_params p) {
    __shared__ float wmax[ALAC_TOP_THREADS / 64];
    const uint32_t row = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
    const uint64_t base = (uint64_t)row * p.lines_per_row * p.line_stride;
    const float* x = p.src + base;
    float* y = p.out + base;
    float m = -INFINITY;
    for (uint32_t k = threadIdx.x; k < p.parts; k += ALAC_TOP_THREADS) m = nan_max(m, p.maxima[(uint64_t)row * p.parts + k]);
    const float mx = block_nan_max(m, wmax);
    const float c = __fsub_rn(mx, p.top);
    for (top_walk w(p, part); w.more(); w.next(p)) {
        const uint64_t at = w.at(p);
        float z = nan_max(x[at], c);
        if (p.relative) z = __fsub_rn(z, mx);
        y[at] = __fadd_rn(__fmul_rn(p.scale, z), p.offset);
    }
}
