// alac_stft.hip -- linear, complex and banded (mel) spectrograms of decoded PCM in one launch (alacgpu_stft_device): framing
// with reflection, the window, two frames per complex N-point transform in LDS (alac_fft_tile.h), the unpacking, power or
// magnitude, an optional banded filterbank and the log.  alac_stft.h states the tile and the LDS layout,
// alac.net_amd/stft.py the arithmetic operation by operation.  Every operation is one IEEE float32 operation, rounded once:
// this file is compiled with -ffp-contract=off, the fused multiply-adds are the ones written, and sqrtf is the correctly
// rounded root (-fhip-fp32-correctly-rounded-divide-sqrt).
#include "alac_stft.h"

#pragma clang fp contract(off)

using namespace alac_fft;

namespace {

// where tap n of frame t reads the plane: one reflection about 0 and about L (L >= N / 2 + 1 brings every index inside)
template <uint32_t N> __device__ inline int64_t tap(uint64_t t, uint32_t hop, uint32_t n, int64_t L) {
    int64_t i = (int64_t)(t * hop) - (int64_t)(N / 2u) + (int64_t)n;
    if (i < 0) i = -i;
    if (i >= L) i = 2 * (L - 1) - i;
    return i;
}

__device__ inline float finish(const alac_stft_params& p, float v) {
    if (p.log_mode != ALAC_STFT_LOG_NONE) {
        v = v < p.floor ? p.floor : v;     // (a NaN stays a NaN, as in np.maximum and torch.clamp)
        v = p.log_mode == ALAC_STFT_LOG_LN ? logf(v) : log10f(v);
    }
    return v;
}

}  // namespace

// Tile blockIdx.x % tiles of plane blockIdx.x / tiles
template <uint32_t N>
__global__ __launch_bounds__(alac_fft_threads(N)) void alac_stft_kernel(alac_stft_params p) {
    constexpr uint32_t K = shape<N>::K, THREADS = shape<N>::THREADS;
    extern __shared__ __align__(16) unsigned char lds[];
    float2* const z = (float2*)lds;                        // [N]
    float* const tileb = (float*)(z + N);                  // [lines][tile + 1]
    const uint32_t stride = p.tile + 1u;
    float* const v = tileb + (size_t)p.lines * stride;     // [2][K], with a filterbank
    const uint64_t plane = blockIdx.x / p.tiles;
    const uint64_t t0 = (uint64_t)(blockIdx.x % p.tiles) * p.tile;
    const uint32_t count = (uint32_t)(p.out_frames - t0 < p.tile ? p.out_frames - t0 : p.tile);
    const float* const x = p.src + plane * p.src_stride;
    const int64_t L = (int64_t)p.frames;
    const bool fb = p.fb_lines != 0u;

    for (uint32_t c = 0; c < count; c += 2u) {
        const bool pair = c + 1u < count;                  // (workgroup-uniform)
        for (uint32_t n = threadIdx.x; n < N; n += THREADS) {
            const float w = p.window[n];
            const float a = __fmul_rn(w, x[tap<N>(t0 + c, p.hop, n, L)]);
            z[n] = make_float2(a, pair ? __fmul_rn(w, x[tap<N>(t0 + c + 1u, p.hop, n, L)]) : 0.0f);
        }
        forward<N>(z, p.table);
        for (uint32_t k = threadIdx.x; k < K; k += THREADS) {
            const float2 zk = z[pos_of<N>(k)], zn = z[pos_of<N>((N - k) & (N - 1u))];
            const float2 A = make_float2(__fmul_rn(0.5f, __fadd_rn(zk.x, zn.x)), __fmul_rn(0.5f, __fsub_rn(zk.y, zn.y)));
            const float2 B = make_float2(__fmul_rn(0.5f, __fadd_rn(zk.y, zn.y)), __fmul_rn(0.5f, __fsub_rn(zn.x, zk.x)));
            if (p.power == ALAC_STFT_COMPLEX) {
                tileb[k * stride + c] = A.x;
                tileb[(K + k) * stride + c] = A.y;
                if (pair) {
                    tileb[k * stride + c + 1u] = B.x;
                    tileb[(K + k) * stride + c + 1u] = B.y;
                }
            } else {
                float va = __fmaf_rn(A.x, A.x, __fmul_rn(A.y, A.y)), vb = __fmaf_rn(B.x, B.x, __fmul_rn(B.y, B.y));
                if (p.power == ALAC_STFT_MAGNITUDE) va = sqrtf(va), vb = sqrtf(vb);
                if (fb) {
                    v[k] = va;
                    v[K + k] = vb;
                } else {
                    tileb[k * stride + c] = finish(p, va);
                    if (pair) tileb[k * stride + c + 1u] = finish(p, vb);
                }
            }
        }
        __syncthreads();                                   // z has been read (the next pair overwrites it); v is whole
        if (fb) {
            const uint32_t both = pair ? 2u : 1u;
            for (uint32_t i = threadIdx.x; i < p.fb_lines * both; i += THREADS) {
                const uint32_t m = i / both, f = i % both;
                uint32_t first = p.bands[3u * m], n = p.bands[3u * m + 1u];
                first = first < K ? first : K;             // (the host has checked the band; nothing outside v is read whatever it holds)
                n = n < K - first ? n : K - first;
                const float* const w = p.weights + p.bands[3u * m + 2u];
                const float* const vf = v + f * K + first;
                float acc = 0.0f;
                for (uint32_t j = 0; j < n; j++) acc = __fmaf_rn(w[j], vf[j], acc);
                tileb[m * stride + c + f] = finish(p, acc);
            }                                              // (v is written again behind the next transform's barriers)
        }
    }
    __syncthreads();
    float* const out = p.out + plane * p.lines * p.out_frames + t0;
    const uint32_t shift = (uint32_t)__ffs((int)p.tile) - 1u;                  // (the tile is a power of two)
    for (uint32_t i = threadIdx.x; i < p.lines << shift; i += THREADS) {
        const uint32_t line = i >> shift, c = i & (p.tile - 1u);
        if (c < count) out[(uint64_t)line * p.out_frames + c] = tileb[line * stride + c];
    }
}

const void* alac_stft_kernel_of(uint32_t n_fft) {
    return n_fft == 256u    ? (const void*)alac_stft_kernel<256u>
           : n_fft == 512u  ? (const void*)alac_stft_kernel<512u>
           : n_fft == 1024u ? (const void*)alac_stft_kernel<1024u>
                            : (const void*)alac_stft_kernel<2048u>;
}
