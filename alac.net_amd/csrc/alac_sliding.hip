// alac_sliding.hip -- Kaldi's sliding-window mean (and variance) normalisation behind the features, one launch.
// include/alacgpu.h states the mathematics, alac_sliding.h the mappings, the ring and the order of the sums.  Every operation is
// one IEEE float32 operation, rounded once: this file is compiled with -ffp-contract=off, the products and sums go through
// __fmul_rn / __fadd_rn / __fsub_rn, the divisions are `/` and the root sqrtf, which
// -fhip-fp32-correctly-rounded-divide-sqrt makes the correctly rounded ones.  src and out may be the same array: a team reads
// every frame of its line into LDS before the chunk that writes it (alac_sliding.h), and no other team touches the line.
#include "alac_sliding.h"

#pragma clang fp contract(off)

namespace {

// The tree of halves over the 64 partials of a wave and over the 16 wave sums of a workgroup: alac_normalize.hip's, whose order
// the pivot shares (that file's helpers are its own: the stage kernels do not include one another)
__device__ inline float wave_sum(float q) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) q = __fadd_rn(q, __shfl_xor(q, h, 64));
    return q;
}

__device__ inline float block_sum(float q, float* wsum) {
    constexpr int WAVES = ALAC_SLIDING_LINE_THREADS / 64;
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

// The tree of halves over the 32 elements of a block, one in each lane of half a wave: q[j] = q[j] + q[j + h], h = 16 .. 1, as a
// butterfly (float addition commutes: lane j and lane j ^ h compute the same value)
__device__ inline float half_wave_sum(float q) {
#pragma unroll
    for (int h = 16; h >= 1; h >>= 1) q = __fadd_rn(q, __shfl_xor(q, h, 64));
    return q;
}

// A line by a team of TEAM threads, `tid` this thread's place in it: 64, a wave (no barrier of its own: the workgroup's waves
// walk the same chunks), or ALAC_SLIDING_LINE_THREADS, the workgroup.  d [ring], b1 and b2 [ring / 32]: the team's LDS.  live:
// the team has a line (every thread of the workgroup comes here for the barriers).
template <int TEAM>
__device__ inline void sliding_line(const alac_sliding_params& p, uint64_t l, bool live, uint32_t tid, float* d, float* b1, float* b2,
                                    float* wsum) {
    const uint64_t n = p.line_len;
    uint64_t v = 0;
    if (live) {
        v = n;
        if (p.valid) {
            const int64_t a = p.valid[l / p.lines_per_row];
            v = a <= 0 ? 0u : ((uint64_t)a < n ? (uint64_t)a : n);
        }
    }
    const float* x = p.src + l * p.line_stride;       // (not touched without `live`)
    float* y = p.out + l * p.line_stride;
    const uint32_t RM = p.ring - 1u, BM = p.ring / ALAC_SLIDING_BLOCK - 1u;
    // the pivot: the mean of the finite elements below v, in alac_normalize.hip's order
    float acc = 0.0f;
    for (uint64_t i = tid; i < v; i += TEAM) {
        const float a = x[i];
        acc = __fadd_rn(acc, isfinite(a) ? a : 0.0f);
    }
    const float sum = TEAM == 64 ? wave_sum(acc) : block_sum(acc, wsum);
    const float pivot = v ? sum / (float)v : 0.0f;
    const uint64_t vr = (v + ALAC_SLIDING_BLOCK - 1u) & ~(uint64_t)(ALAC_SLIDING_BLOCK - 1u);      // the blocks with a valid frame
    const bool whole = n <= p.ring;
    uint64_t loaded = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += TEAM) {
        // d and the block sums up to where this chunk's windows reach: e <= t + window
        uint64_t need = vr;
        if (!whole) {
            const uint64_t reach = (c0 + TEAM + p.window + ALAC_SLIDING_BLOCK - 1u) & ~(uint64_t)(ALAC_SLIDING_BLOCK - 1u);
            need = reach < vr ? reach : vr;
        }
        if (need < loaded) need = loaded;
        __syncthreads();                                          // the chunk before is done with what the ring gives up
        for (uint64_t i = loaded + tid; i < need; i += TEAM) d[(uint32_t)i & RM] = i < v ? __fsub_rn(x[i], pivot) : 0.0f;
        __syncthreads();
        const uint64_t blk0 = loaded / ALAC_SLIDING_BLOCK, blk1 = need / ALAC_SLIDING_BLOCK;
        for (uint64_t b = blk0 + 2u * (tid >> 6); b < blk1; b += TEAM / 32) {      // (b is the wave's: two blocks a turn)
            const uint64_t blk = b + ((tid >> 5) & 1u);
            const bool has = blk < blk1;
            const float q = has ? d[((uint32_t)blk * ALAC_SLIDING_BLOCK + (tid & 31u)) & RM] : 0.0f;
            const float s1 = half_wave_sum(q);
            if (has && (tid & 31u) == 0u) b1[(uint32_t)blk & BM] = s1;
            if (p.norm_vars) {
                const float s2 = half_wave_sum(__fmul_rn(q, q));
                if (has && (tid & 31u) == 0u) b2[(uint32_t)blk & BM] = s2;
            }
        }
        loaded = need;
        __syncthreads();
        const uint64_t t = c0 + tid;
        if (!live || t >= n) continue;
        float r = 0.0f;
        if (t < v) {
            // Kaldi's window of frame t, its quirks included
            const int64_t T = (int64_t)t, V = (int64_t)v, W = p.window;
            int64_t s, e;
            if (p.center) {
                s = T - W / 2;
                e = s + W;
            } else {
                s = T - W;
                e = T + 1;
            }
            if (s < 0) {
                e -= s;
                s = 0;
            }
            if (!p.center && e > T) e = T + 1 > (int64_t)p.min_window ? T + 1 : (int64_t)p.min_window;
            if (e > V) {
                s -= e - V;
                e = V;
                if (s < 0) s = 0;
            }
            const int64_t N = e - s, j0 = (s + 31) >> 5, j1 = e >> 5;
            const int64_t head_end = j0 < j1 ? 32 * j0 : e;
            float S1 = 0.0f, S2 = 0.0f;
            for (int64_t i = s; i < head_end; i++) {
                const float a = d[(uint32_t)i & RM];
                S1 = __fadd_rn(S1, a);
                if (p.norm_vars) S2 = __fadd_rn(S2, __fmul_rn(a, a));
            }
            if (j0 < j1) {
                for (int64_t j = j0; j < j1; j++) {
                    S1 = __fadd_rn(S1, b1[(uint32_t)j & BM]);
                    if (p.norm_vars) S2 = __fadd_rn(S2, b2[(uint32_t)j & BM]);
                }
                for (int64_t i = 32 * j1; i < e; i++) {
                    const float a = d[(uint32_t)i & RM];
                    S1 = __fadd_rn(S1, a);
                    if (p.norm_vars) S2 = __fadd_rn(S2, __fmul_rn(a, a));
                }
            }
            const float fN = (float)N;
            const float m = S1 / fN;
            r = __fsub_rn(d[(uint32_t)t & RM], m);
            if (p.norm_vars) {
                float var = __fsub_rn(S2 / fN, __fmul_rn(m, m));
                var = var < ALAC_SLIDING_VAR_FLOOR ? ALAC_SLIDING_VAR_FLOOR : var;          // (a NaN stays one, as np.maximum's)
                r = N == 1 ? 0.0f : r / sqrtf(var);
            }
        }
        y[t] = r;
    }
}

}  // namespace

// A wave per line of at most ALAC_SLIDING_WAVE_MAX frames, ALAC_SLIDING_WAVE_LINES lines per workgroup
__global__ __launch_bounds__(ALAC_SLIDING_WAVE_THREADS) void alac_sliding_wave_kernel(alac_sliding_params p) {
    extern __shared__ float lds[];
    const uint32_t wave = threadIdx.x >> 6, blocks = p.ring / ALAC_SLIDING_BLOCK;
    float* const d = lds + wave * (p.ring + 2u * blocks);
    const uint64_t l = (uint64_t)blockIdx.x * ALAC_SLIDING_WAVE_LINES + wave;
    sliding_line<64>(p, l, l < p.lines, threadIdx.x & 63u, d, d + p.ring, d + p.ring + blocks, nullptr);
}

// A workgroup per longer line
__global__ __launch_bounds__(ALAC_SLIDING_LINE_THREADS) void alac_sliding_line_kernel(alac_sliding_params p) {
    extern __shared__ float lds[];
    const uint32_t blocks = p.ring / ALAC_SLIDING_BLOCK;
    sliding_line<ALAC_SLIDING_LINE_THREADS>(p, blockIdx.x, true, threadIdx.x, lds, lds + p.ring, lds + p.ring + blocks,
                                            lds + p.ring + 2u * blocks);
}
