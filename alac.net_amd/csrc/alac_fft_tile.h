// alac_fft_tile.h -- the N-point complex transform of a workgroup in LDS, shared by the phase vocoder (alac_stretch.hip) and the
// STFT (alac_stft.hip): N = 256, 512, 1024 or 2048, z[N] float2 in LDS, alac_fft_threads(N) threads.  Every operation is one
// IEEE float32 operation, rounded once (__fmul_rn / __fadd_rn / __fsub_rn): a file that includes this is compiled with
// -ffp-contract=off.  alac_stretch.h states the stages, alac.net_amd/pitch.py restates them operation by operation (`_forward`,
// `_inverse`, `positions`, `twiddles`).
//
// For N = 512 and 2048 a radix-2 decimation-in-frequency stage (q < N / 2: a = z[q], b = z[q + N / 2]; z[q] = a + b,
// z[q + N / 2] = (a - b) tw[q]) and then radix-4 stages of span L = N / 8 .. 1 over both halves; for 256 and 1024 the radix-4
// stages from L = N / 4.  tw[k] = exp(-2 pi i k / N), made by the host in float64 and rounded once.  Bin k ends at pos_of<N>(k):
// the base-4 digits of k (of k / 2, in the half k % 2 names) reversed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ constexpr uint32_t alac_fft_threads(uint32_t n_fft) { return n_fft / 4u < 256u ? n_fft / 4u : 256u; }

namespace alac_fft {

__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)); }
__device__ inline float2 cmul(float2 a, float2 b) {
    return make_float2(__fsub_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fadd_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x)));
}
__device__ inline float2 conj(float2 a) { return make_float2(a.x, -a.y); }

template <uint32_t N> struct shape {
    static_assert(N == 256u || N == 512u || N == 1024u || N == 2048u, "n_fft is 256, 512, 1024 or 2048");
    static constexpr uint32_t H = N / 4u, K = N / 2u + 1u, THREADS = alac_fft_threads(N);
    static constexpr bool ODD = N == 512u || N == 2048u;      // a radix-2 stage in front of the radix-4 stages
    static constexpr uint32_t DIGITS = N <= 512u ? 4u : 5u;   // the base-4 digits behind it
    static constexpr uint32_t L0 = ODD ? N / 8u : N / 4u;     // the first radix-4 span
    static_assert(H % THREADS == 0u, "a thread's elements of a frame fall on its own elements of a tile");
};

// where bin k of the forward transform lies
template <uint32_t N> __device__ inline uint32_t pos_of(uint32_t k) {
    uint32_t kk = shape<N>::ODD ? k >> 1 : k, rev = 0u;
#pragma unroll
    for (uint32_t d = 0; d < shape<N>::DIGITS; d++) {
        rev = (rev << 2) | (kk & 3u);
        kk >>= 2;
    }
    return shape<N>::ODD ? (k & 1u) * (N / 2u) + rev : rev;
}

// The forward transform of z[N] in LDS, in place, natural order in, bin k at pos_of(k) out.  A butterfly reads and writes its
// own elements; a barrier stands in front of every stage and behind the last.
template <uint32_t N> __device__ inline void forward(float2* z, const float2* tw) {
    constexpr uint32_t THREADS = shape<N>::THREADS;
    if (shape<N>::ODD) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < N / 2u; q += THREADS) {
            const float2 a = z[q], b = z[q + N / 2u];
            z[q] = cadd(a, b);
            z[q + N / 2u] = cmul(csub(a, b), tw[q]);
        }
    }
    for (uint32_t L = shape<N>::L0; L >= 1u; L >>= 2) {
        const uint32_t step = N / (4u * L);
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < N / 4u; q += THREADS) {
            const uint32_t j = q & (L - 1u), i0 = ((q - j) << 2) + j;
            const float2 a = z[i0], b = z[i0 + L], c = z[i0 + 2u * L], d = z[i0 + 3u * L];
            const float2 t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), bd = csub(b, d);
            const float2 t3 = make_float2(bd.y, -bd.x);                       // -i (b - d)
            z[i0] = cadd(t0, t2);
            z[i0 + L] = cmul(cadd(t1, t3), tw[j * step]);
            z[i0 + 2u * L] = cmul(csub(t0, t2), tw[2u * j * step]);
            z[i0 + 3u * L] = cmul(csub(t1, t3), tw[3u * j * step]);
        }
    }
    __syncthreads();
}

// The inverse transform, not divided by N: bin k at pos_of(k) in, natural order out; the forward stages' conjugate transposes
// in the opposite order
template <uint32_t N> __device__ inline void inverse(float2* z, const float2* tw) {
    constexpr uint32_t THREADS = shape<N>::THREADS;
    for (uint32_t L = 1u; L <= shape<N>::L0; L <<= 2) {
        const uint32_t step = N / (4u * L);
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < N / 4u; q += THREADS) {
            const uint32_t j = q & (L - 1u), i0 = ((q - j) << 2) + j;
            const float2 z0 = z[i0], z1 = cmul(z[i0 + L], conj(tw[j * step])), z2 = cmul(z[i0 + 2u * L], conj(tw[2u * j * step])),
                         z3 = cmul(z[i0 + 3u * L], conj(tw[3u * j * step]));
            const float2 u0 = cadd(z0, z2), u1 = csub(z0, z2), u2 = cadd(z1, z3), dz = csub(z1, z3);
            const float2 u3 = make_float2(-dz.y, dz.x);                       // i (z1 - z3)
            z[i0] = cadd(u0, u2);
            z[i0 + L] = cadd(u1, u3);
            z[i0 + 2u * L] = csub(u0, u2);
            z[i0 + 3u * L] = csub(u1, u3);
        }
    }
    if (shape<N>::ODD) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < N / 2u; q += THREADS) {
            const float2 a = z[q], b = cmul(z[q + N / 2u], conj(tw[q]));
            z[q] = cadd(a, b);
            z[q + N / 2u] = csub(a, b);
        }
    }
    __syncthreads();
}

}  // namespace alac_fft
