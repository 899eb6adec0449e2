// alac_stretch.hip -- time stretch of the crops with the pitch kept, a phase vocoder in three launches: analyse (the STFT of
// every live row: reflect padding, the periodic Hann window, an N-point transform in LDS), scan (one lane per bin walks the
// output frames: magnitudes interpolated, the phase carried as a unit phasor -- no angle is taken) and synthesise (the inverse
// transforms of the frames that cover a tile of output, windowed, overlap-added in ascending frame order out of LDS and divided
// by the envelope), no atomics.  include/alacgpu.h states the arithmetic, alac_stretch.h the transform, the layouts and the
// order of the sums.  Every operation is one IEEE float32 operation, rounded once: this file is compiled with -ffp-contract=off
// and the products and sums go through __fmul_rn / __fadd_rn / __fsub_rn; the division is `/` and the root sqrtf, which
// -fhip-fp32-correctly-rounded-divide-sqrt makes the correctly rounded ones.  The copy of rows that the pitch shift ends with
// is here too.  The transform itself (shape, pos_of, forward, inverse) is alac_fft_tile.h's, which alac_stft.hip runs too.
#include "alac_stretch.h"
#include "alac_fft_tile.h"

#pragma clang fp contract(off)

using namespace alac_fft;
static_assert(alac_stretch_threads(512u) == alac_fft_threads(512u) && alac_stretch_threads(1024u) == alac_fft_threads(1024u) &&
              alac_stretch_threads(2048u) == alac_fft_threads(2048u), "the transform's threads are the launch's");

namespace {

__device__ inline float cabs(float2 a) { return sqrtf(__fadd_rn(__fmul_rn(a.x, a.x), __fmul_rn(a.y, a.y))); }
// z / |z|, 1 where |z| is not above 0 (a NaN too)
__device__ inline float2 phasor(float2 a) {
    const float m = cabs(a);
    return m > 0.0f ? make_float2(a.x / m, a.y / m) : make_float2(1.0f, 0.0f);
}

// A row's integers (alac_stretch.h); workgroup-uniform
struct row_state {
    int64_t given;                // valid[row] as it is, frames without `valid`
    uint64_t v, T, Tp, Ls;        // the valid frames; of a live row the STFT frames, the output frames, the output samples
    uint32_t p, q;
    bool live;
};

template <uint32_t N> __device__ inline row_state row_of(const alac_stretch_params& s, uint32_t row) {
    row_state r;
    r.given = s.valid ? s.valid[row] : (int64_t)s.frames;
    r.v = r.given <= 0 ? 0u : ((uint64_t)r.given < s.frames ? (uint64_t)r.given : s.frames);
    const int32_t p = s.p[row], q = s.q[row];
    r.live = p > 0 && q > 0 && p != q && (uint32_t)p <= ALAC_STRETCH_MAX_TERM && (uint32_t)q <= ALAC_STRETCH_MAX_TERM && r.v > N / 2u;
    r.p = (uint32_t)p;
    r.q = (uint32_t)q;
    r.T = r.Tp = r.Ls = 0u;
    if (r.live) {                 // (frames is below 2^40: the products fit)
        r.T = alac_stretch_frames(r.v, N);
        r.Tp = (r.T * r.p + r.q - 1u) / r.q;
        r.Ls = (2u * r.v * r.p + r.q) / (2u * r.q);
    }
    return r;
}

}  // namespace

// Frame blockIdx.x % t_max of plane blockIdx.x / t_max: the spectrum of the reflected, windowed frame.  The workgroup of frame 0
// of a row's channel 0 writes the row's new length, live or not.
template <uint32_t N>
__global__ __launch_bounds__(alac_stretch_threads(N)) void alac_stretch_analyse_kernel(alac_stretch_params s) {
    constexpr uint32_t H = shape<N>::H, K = shape<N>::K, THREADS = shape<N>::THREADS;
    __shared__ __align__(16) float2 z[N];
    const uint64_t plane = blockIdx.x / s.t_max;
    const uint32_t t = blockIdx.x % s.t_max;
    const uint32_t row = (uint32_t)(plane / s.channels);
    const row_state r = row_of<N>(s, row);
    if (t == 0u && plane % s.channels == 0u && threadIdx.x == 0u) {
        const int64_t kept = r.given < (int64_t)s.frames ? r.given : (int64_t)s.frames;
        s.valid_out[row] = r.live ? (int64_t)(r.Ls < s.out_frames ? r.Ls : s.out_frames) : kept;
    }
    if (!r.live || t >= r.T) return;                      // (the workgroup's: every thread returns or none)
    const float* x = s.src + plane * s.src_stride;
    for (uint32_t n = threadIdx.x; n < N; n += THREADS) {
        int64_t i = (int64_t)t * H - (int64_t)(N / 2u) + (int64_t)n;       // below v + N / 2, and v > N / 2: one reflection each way
        if (i < 0) i = -i;
        if (i >= (int64_t)r.v) i = 2 * ((int64_t)r.v - 1) - i;
        z[n] = make_float2(__fmul_rn(s.window[n], x[i]), 0.0f);
    }
    forward<N>(z, s.table);
    float2* const X = s.X + ((uint64_t)plane * s.t_max + t) * K;
    for (uint32_t k = threadIdx.x; k < K; k += THREADS) X[k] = z[pos_of<N>(k)];
}

// Lane blockIdx.x * THREADS + threadIdx.x is bin k of a plane: the output frames in ascending order
template <uint32_t N>
__global__ __launch_bounds__(ALAC_STRETCH_SCAN_THREADS) void alac_stretch_scan_kernel(alac_stretch_params s) {
    constexpr uint32_t K = shape<N>::K;
    const uint64_t lane = (uint64_t)blockIdx.x * ALAC_STRETCH_SCAN_THREADS + threadIdx.x;
    if (lane >= s.chains) return;
    const uint64_t plane = lane / K;
    const uint32_t k = (uint32_t)(lane % K);
    const row_state r = row_of<N>(s, (uint32_t)(plane / s.channels));
    if (!r.live) return;
    const float2* const X = s.X + plane * s.t_max * K + k;
    float2* const Y = s.Y + plane * s.t_cap * K + k;
    const uint64_t count = r.Tp < s.t_cap ? r.Tp : s.t_cap;
    const float2 zero = make_float2(0.0f, 0.0f);
    float2 P = phasor(X[0]);
    uint64_t i = 0;                                        // (j q) / p
    uint32_t num = 0;                                      // (j q) % p
    for (uint64_t j = 0; j < count; j++) {
        const float2 a = i < r.T ? X[i * K] : zero, b = i + 1u < r.T ? X[(i + 1u) * K] : zero;
        const float alpha = (float)num / (float)r.p;
        const float mag = __fadd_rn(__fmul_rn(alpha, cabs(b)), __fmul_rn(__fsub_rn(1.0f, alpha), cabs(a)));
        Y[j * K] = make_float2(__fmul_rn(mag, P.x), __fmul_rn(mag, P.y));
        P = phasor(cmul(P, cmul(phasor(b), conj(phasor(a)))));
        num += r.q;                                        // (below 2^21)
        i += num / r.p;
        num %= r.p;
    }
}

// Tile blockIdx.x % out_tiles of plane blockIdx.x / out_tiles: ALAC_STRETCH_TILE_HOPS hops of the output of a live row
template <uint32_t N>
__global__ __launch_bounds__(alac_stretch_threads(N)) void alac_stretch_synth_kernel(alac_stretch_params s) {
    constexpr uint32_t H = shape<N>::H, K = shape<N>::K, THREADS = shape<N>::THREADS, G = ALAC_STRETCH_TILE_HOPS, TILE = G * H;
    __shared__ __align__(16) float2 z[N];
    __shared__ float acc[TILE];
    const uint64_t plane = blockIdx.x / s.out_tiles;
    const uint32_t m = blockIdx.x % s.out_tiles;
    const row_state r = row_of<N>(s, (uint32_t)(plane / s.channels));
    if (!r.live) return;                                   // (the workgroup's: every thread returns or none)
    const uint64_t n0 = (uint64_t)m * TILE;
    const uint64_t count = r.Tp < s.t_cap ? r.Tp : s.t_cap;   // the frames there are
    uint64_t last = (r.Tp - 1u) * H + 1u;                  // the samples that are computed: n <= (T' - 1) H, below Ls and out_frames
    last = last < r.Ls ? last : r.Ls;
    last = last < s.out_frames ? last : s.out_frames;
    float* const y = s.out + plane * s.out_stride;
    for (uint32_t t = threadIdx.x; t < TILE; t += THREADS) acc[t] = 0.0f;      // (a thread's own elements, here and below)
    if (n0 < last) {
        const float2* const Y = s.Y + plane * s.t_cap * K;
        const int64_t j0 = (int64_t)m * G - 1;
        for (int64_t j = j0 < 0 ? 0 : j0; j < j0 + (int64_t)(G + 3u) && (uint64_t)j < count; j++) {
            __syncthreads();                               // the frame before has been read
            for (uint32_t k = threadIdx.x; k < K; k += THREADS) {
                const float2 a = Y[(uint64_t)j * K + k];
                if (k == 0u || k == N / 2u) {
                    z[pos_of<N>(k)] = make_float2(a.x, 0.0f);
                } else {
                    z[pos_of<N>(k)] = a;
                    z[pos_of<N>(N - k)] = conj(a);
                }
            }
            inverse<N>(z, s.table);
            const int64_t shift = (j - (int64_t)m * G - 2) * (int64_t)H;      // the tile's element of the frame's element 0
            for (uint32_t i = threadIdx.x; i < N; i += THREADS) {
                const int64_t at = shift + (int64_t)i;
                if (at >= 0 && at < (int64_t)TILE)
                    acc[at] = __fadd_rn(acc[at], __fmul_rn(s.window[i], __fmul_rn(z[i].x, 1.0f / (float)N)));
            }
        }
    }
    for (uint32_t t = threadIdx.x; t < TILE; t += THREADS) {
        const uint64_t n = n0 + t;
        if (n >= s.out_frames) break;
        float value = 0.0f;
        if (n < last) {
            float env = 0.0f;
            const int64_t hop = (int64_t)(n / H);
            for (int64_t j = hop - 1; j <= hop + 2; j++) {
                if (j < 0 || (uint64_t)j >= count) continue;
                const float w = s.window[n + 2u * H - (uint64_t)j * H];
                env = __fadd_rn(env, __fmul_rn(w, w));
            }
            value = acc[t] / env;
        }
        y[n] = value;
    }
}

void alac_stretch_kernels(uint32_t n_fft, const void*& analyse, const void*& scan, const void*& synth) {
    if (n_fft == 512u) {
        analyse = (const void*)alac_stretch_analyse_kernel<512u>, scan = (const void*)alac_stretch_scan_kernel<512u>;
        synth = (const void*)alac_stretch_synth_kernel<512u>;
    } else if (n_fft == 1024u) {
        analyse = (const void*)alac_stretch_analyse_kernel<1024u>, scan = (const void*)alac_stretch_scan_kernel<1024u>;
        synth = (const void*)alac_stretch_synth_kernel<1024u>;
    } else {
        analyse = (const void*)alac_stretch_analyse_kernel<2048u>, scan = (const void*)alac_stretch_scan_kernel<2048u>;
        synth = (const void*)alac_stretch_synth_kernel<2048u>;
    }
}

// Tile blockIdx.x % tiles of plane blockIdx.x / tiles: the frames below the row's valid count, from src to out
__global__ __launch_bounds__(ALAC_STRETCH_COPY_THREADS) void alac_copy_rows_kernel(alac_copy_rows_params p) {
    const uint64_t plane = blockIdx.x / p.tiles;
    const uint64_t first = (uint64_t)(blockIdx.x % p.tiles) * ALAC_STRETCH_COPY_TILE;
    const int64_t a = p.valid[plane / p.channels];
    const uint64_t v = a <= 0 ? 0u : ((uint64_t)a < p.frames ? (uint64_t)a : p.frames);
    const uint64_t end = first + ALAC_STRETCH_COPY_TILE < v ? first + ALAC_STRETCH_COPY_TILE : v;
    const float* const x = p.src + plane * p.src_stride;
    float* const y = p.out + plane * p.out_stride;
    for (uint64_t n = first + threadIdx.x; n < end; n += ALAC_STRETCH_COPY_THREADS) y[n] = x[n];
}
