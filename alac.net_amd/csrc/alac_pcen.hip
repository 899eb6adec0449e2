// alac_pcen.hip -- per-channel energy normalisation behind the features: the first-order smoother of every line as a blocked
// scan and the compression of every frame, one launch.  include/alacgpu.h states the mathematics, alac_pcen.h the mappings, the
// order of the operations and the two polynomials.  Every operation is one IEEE float32 operation, rounded once: this file is
// compiled with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt.  src and out may be the same array: a lane reads
// its frames of a pass before it writes them, and no other lane touches them.
#include "alac_pcen.h"

#pragma clang fp contract(off)

namespace {

// CHUNK frames of a line: a line begins wherever line_stride puts it, so the vector is aligned as its elements are
typedef float chunk_t __attribute__((ext_vector_type(4), aligned(4)));
static_assert(ALAC_PCEN_CHUNK == 4u, "chunk_t is a lane's frames of a pass");

// A line by a team of WAVES waves, `tid` this thread's place in it.  wtot [WAVES]: the workgroup team's LDS (WAVES > 1; every
// thread of the workgroup has the same line, so the barriers are met by all).  live: the wave has a line.
template <int WAVES>
__device__ inline void pcen_line(const alac_pcen_params& p, uint64_t l, bool live, uint32_t tid, float2* wtot) {
    constexpr uint32_t CHUNK = ALAC_PCEN_CHUNK, PASS = 64u * WAVES * CHUNK;
    if (!live) return;                                    // (WAVES == 1 only: no barrier below)
    const uint64_t n = p.line_len;
    uint64_t v = n;
    if (p.valid) {
        const int64_t a = p.valid[l / p.lines_per_row];
        v = a <= 0 ? 0u : ((uint64_t)a < n ? (uint64_t)a : n);
    }
    float b = p.b, gain = p.gain, bias = p.bias, power = p.power, bias_pow = p.bias_pow;
    if (p.table) {
        const uint32_t j = (uint32_t)(l % p.lines_per_param), L = p.lines_per_param;
        b = p.table[j];
        gain = p.table[L + j];
        bias = p.table[2u * L + j];
        power = p.table[3u * L + j];
        bias_pow = p.table[4u * L + j];
    }
    const float a = 1.0f - b, neg_gain = -gain;
    const float* x = p.src + l * p.line_stride;
    float* y = p.out + l * p.line_stride;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    float carry = 0.0f;
    for (uint64_t p0 = 0; p0 < n; p0 += PASS) {
        const uint64_t t0 = p0 + (uint64_t)tid * CHUNK;
        float r[CHUNK] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p0 < v) {                                     // (the same for the whole team)
            float s[CHUNK] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (t0 + CHUNK <= v) {
                const chunk_t q = *(const chunk_t*)(x + t0);
#pragma unroll
                for (uint32_t k = 0; k < CHUNK; k++) s[k] = p.scale * q[k];
            } else {
#pragma unroll
                for (uint32_t k = 0; k < CHUNK; k++)
                    if (t0 + k < v) s[k] = p.scale * x[t0 + k];
            }
            // the lane's own frames from m = 0, and its map
            float mk[CHUNK], Ak[CHUNK];
            float m = 0.0f, A = 1.0f;
#pragma unroll
            for (uint32_t k = 0; k < CHUNK; k++) {
                const uint64_t t = t0 + k;
                if (t == 0u) {
                    m = s[k];
                    A = 0.0f;
                } else if (t < v) {
                    m = a * m + b * s[k];
                    A = A * a;
                }
                mk[k] = m;
                Ak[k] = A;
            }
            // the wave's inclusive scan of the maps
            float IA = A, IB = m;
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const float pa = __shfl_up(IA, d, 64), pb = __shfl_up(IB, d, 64);
                if (lane >= d) {
                    IB = IA * pb + IB;
                    IA = IA * pa;
                }
            }
            const float EA = __shfl_up(IA, 1u, 64), EB = __shfl_up(IB, 1u, 64);
            float wc = carry, next;
            if (WAVES == 1) {
                next = __shfl(IA, 63, 64) * carry + __shfl(IB, 63, 64);
            } else {
                if (lane == 63u) wtot[wave] = make_float2(IA, IB);
                __syncthreads();
                next = carry;
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)WAVES; j++) {
                    if (j == wave) wc = next;
                    const float2 w = wtot[j];
                    next = w.x * next + w.y;
                }
                __syncthreads();                          // (the next pass writes wtot again)
            }
            carry = next;
            const float C = lane == 0u ? wc : EA * wc + EB;
#pragma unroll
            for (uint32_t k = 0; k < CHUNK; k++) {
                if (t0 + k >= v) continue;
                const float M = Ak[k] * C + mk[k];
                if (p.stage) {
                    r[k] = M;
                } else {
                    const float u = p.eps + M;
                    const float g = alac_pcen_exp2(neg_gain * alac_pcen_log2(u));
                    const float w = s[k] * g + bias;
                    r[k] = alac_pcen_exp2(power * alac_pcen_log2(w)) - bias_pow;
                }
            }
        }
        if (t0 + CHUNK <= n) {
            chunk_t q;
#pragma unroll
            for (uint32_t k = 0; k < CHUNK; k++) q[k] = r[k];
            *(chunk_t*)(y + t0) = q;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < CHUNK; k++)
                if (t0 + k < n) y[t0 + k] = r[k];
        }
    }
}

}  // namespace

// A wave per line of at most ALAC_PCEN_WAVE_MAX frames, ALAC_PCEN_WAVE_LINES lines per workgroup
__global__ __launch_bounds__(ALAC_PCEN_WAVE_THREADS) void alac_pcen_wave_kernel(alac_pcen_params p) {
    const uint64_t l = (uint64_t)blockIdx.x * ALAC_PCEN_WAVE_LINES + (threadIdx.x >> 6);
    pcen_line<1>(p, l, l < p.lines, threadIdx.x & 63u, nullptr);
}

// A workgroup per longer line
__global__ __launch_bounds__(ALAC_PCEN_LINE_THREADS) void alac_pcen_line_kernel(alac_pcen_params p) {
    __shared__ float2 wtot[ALAC_PCEN_LINE_THREADS / 64];
    pcen_line<ALAC_PCEN_LINE_THREADS / 64>(p, blockIdx.x, true, threadIdx.x, wtot);
}
