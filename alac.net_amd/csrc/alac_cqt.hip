// alac_cqt.hip -- constant-Q features of decoded PCM in one launch (alacgpu_cqt_device): every bin's own kernel against the
// signal as a ragged GEMM on the exact-f32 MFMA, magnitude or power, and the log (alac.net_amd/cqt.py states the mathematics,
// alac_cqt.h the layout).  Compiled with -ffp-contract=off and the correctly rounded root: every multiply-add here is a
// __builtin_fmaf or the MFMA builtin, so the twin of cqt.py can repeat it operation by operation.
#include "alac_cqt.h"

namespace {

constexpr uint32_t AHEAD = 8u;   // k-steps (of two taps) whose table fragments are loaded ahead of their MFMAs

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// What is stored for a bin's sums
__device__ __forceinline__ float finish(const alac_cqt_params& p, float re, float im) {
    float v = __builtin_fmaf(re, re, im * im);
    if (p.power == 1u) v = __builtin_sqrtf(v);
    if (p.log_mode != ALAC_CQT_LOG_NONE) {
        v = v < p.floor ? p.floor : v;     // (a NaN stays a NaN, as in np.maximum and torch.clamp)
        v = p.log_mode == ALAC_CQT_LOG_LN ? logf(v) : log10f(v);
    }
    return v;
}

}  // namespace

__global__ __launch_bounds__(ALAC_CQT_THREADS) void alac_cqt_kernel(alac_cqt_params p) {
    extern __shared__ __align__(16) float xs[];
    const uint32_t tid = threadIdx.x;
    const uint32_t hop = p.hop;
    const uint32_t tile_i = blockIdx.x % p.tiles;
    const uint64_t plane = blockIdx.x / p.tiles;
    const uint64_t t0 = (uint64_t)tile_i * p.tile;
    const uint64_t left = p.out_frames - t0;
    const uint32_t nt = left < p.tile ? (uint32_t)left : p.tile;      // the tile's frames
    const uint32_t skew = alac_cqt_skew(hop, p.tile);
    const float* const src = p.src + plane * p.src_stride;
    float* const out = p.out + plane * p.n_bins * p.out_frames + t0;

    // the span of the tile's frames: frame t of the tile covers [t hop, t hop + n0 + 1) of it, sample 0 of the span is sample
    // t0 hop - c0 of the plane; zeros outside the signal, and nothing is read there
    const int64_t s_lo = (int64_t)(t0 * hop) - (int64_t)p.c0;
    const int64_t L = (int64_t)p.frames;
    const uint32_t span = (nt - 1u) * hop + p.n0 + 1u;
    int bad = 0;
    for (uint32_t idx = tid; idx < span; idx += ALAC_CQT_THREADS) {
        const int64_t g = s_lo + (int64_t)idx;
        const float v = (g >= 0 && g < L) ? src[g] : 0.0f;
        bad |= finite(v) ? 0 : 1;
        xs[idx + skew * (idx / hop)] = v;
    }
    bad = __syncthreads_or(bad);

    if (!bad) {
        // D = G . frames^T, a block of 16 bins per accumulator; the lane's frame is t, its tap of a k-step 2 s + h
        const uint32_t lane = tid & 63u, t = tid & 31u, h = (tid >> 5) & 1u, wave = tid >> 6;
        const bool frame_ok = t < nt;
        const uint32_t xbase = frame_ok ? t * (hop + skew) : 0u;
        for (uint32_t blk = wave; blk < p.n_blocks; blk += ALAC_CQT_THREADS / 64u) {
            const uint32_t steps = p.blk_k[blk] / 2u;
            const float* a = p.table + p.blk_off[blk] + lane;         // a k-step's fragments: 64 neighbouring floats
            // the lane's tap, m = blk_start + 2 s + h of the frame's span, lives at xbase + m + skew (m / hop)
            const uint32_t m0 = p.blk_start[blk] + h;
            uint32_t r = m0 % hop;
            uint32_t addr = xbase + m0 + skew * (m0 / hop);
            f32x16 acc = {};
            float cur[AHEAD], nxt[AHEAD];
            uint32_t s = 0;
            if (steps >= AHEAD) {
#pragma unroll
                for (uint32_t u = 0; u < AHEAD; ++u) cur[u] = a[u * 64u];
                a += AHEAD * 64u;
            }
            for (; s + AHEAD <= steps; s += AHEAD) {
                const bool more = s + 2u * AHEAD <= steps;            // (uniform: a whole group behind this one)
                if (more) {
#pragma unroll
                    for (uint32_t u = 0; u < AHEAD; ++u) nxt[u] = a[u * 64u];
                    a += AHEAD * 64u;
                }
#pragma unroll
                for (uint32_t u = 0; u < AHEAD; ++u) {
                    const float b = frame_ok ? xs[addr] : 0.0f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u], b, acc, 0, 0, 0);
                    addr += 2u;
                    r += 2u;
                    if (r >= hop) {      // (an odd hop has no skew, and whatever r does there changes nothing)
                        r -= hop;
                        addr += skew;
                    }
                }
                if (more) {
#pragma unroll
                    for (uint32_t u = 0; u < AHEAD; ++u) cur[u] = nxt[u];
                }
            }
            for (; s < steps; ++s) {     // what is left: up to AHEAD - 1 k-steps
                const float va = a[0];
                a += 64u;
                const float b = frame_ok ? xs[addr] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va, b, acc, 0, 0, 0);
                addr += 2u;
                r += 2u;
                if (r >= hop) {
                    r -= hop;
                    addr += skew;
                }
            }
            // D's register j of this lane is row (j & 3) + 8 (j >> 2) + 4 h of the block, frame t: registers j and j + 4 are
            // the real and the imaginary part of the block's bin 8 (j >> 3) + 4 h + (j & 3)
            if (frame_ok) {
#pragma unroll
                for (uint32_t j = 0; j < 16u; ++j) {
                    if (j & 4u) continue;
                    const uint32_t bin = blk * ALAC_CQT_BLOCK_BINS + 8u * (j >> 3) + 4u * h + (j & 3u);
                    if (bin < p.n_bins) out[(uint64_t)bin * p.out_frames + t] = finish(p, acc[j], acc[j + 4u]);
                }
            }
        }
        return;
    }

    // The second path: the span holds a value that is not finite.  Element (bin, frame) is its own two chains over the
    // bin's own taps, ascending, on the VALU: what the MFMA computes where every sample is finite, and IEEE's answer here.
    for (uint32_t e = tid; e < p.n_bins * nt; e += ALAC_CQT_THREADS) {
        const uint32_t bin = e / nt, t = e % nt;
        const uint32_t blk = bin / ALAC_CQT_BLOCK_BINS, j = bin % ALAC_CQT_BLOCK_BINS;
        const uint32_t K = p.blk_k[blk];
        const uint32_t cb = p.c0 - p.blk_start[blk];                  // c of the block's longest kernel
        uint32_t N = p.lengths[bin];
        N = N < K ? N : K;                                            // (the table's own limits, whatever `lengths` holds)
        const uint32_t at = cb > N / 2u ? cb - N / 2u : 0u;           // the bin's first tap among the block's K
        if (at + N > K) N = K - at;
        const float* a = p.table + p.blk_off[blk] + (size_t)at * 32u + (j >> 3) * 16u + (j & 7u);
        const uint32_t m0 = p.blk_start[blk] + at;
        uint32_t r = m0 % hop;
        uint32_t addr = t * (hop + skew) + m0 + skew * (m0 / hop);
        float re = 0.0f, im = 0.0f;
        for (uint32_t n = 0; n < N; ++n) {
            const float x = xs[addr];
            re = __builtin_fmaf(a[0], x, re);
            im = __builtin_fmaf(a[8], x, im);
            a += 32u;
            addr += 1u;
            r += 1u;
            if (r >= hop) {
                r -= hop;
                addr += skew;
            }
        }
        out[(uint64_t)bin * p.out_frames + t] = finish(p, re, im);
    }
}
