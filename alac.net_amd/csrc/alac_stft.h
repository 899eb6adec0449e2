// alac_stft.h -- the STFT kernel (alac_stft.hip): its launch parameters, its tile and its LDS layout, shared with the C ABI
// (alacgpu_stages.hip).  alac.net_amd/stft.py states the arithmetic operation by operation and builds the tables;
// alac_fft_tile.h is the transform.
//
// N = n_fft is 256, 512, 1024 or 2048, K = N / 2 + 1 bins.  The output [planes, lines, T'] has time as its last dimension, so
// a workgroup (alac_fft_threads(N) threads) owns a tile of consecutive frames of one plane, beginning on an even frame, and
// stores whole runs of a line.  Frames 2 j and 2 j + 1 of the plane are one complex transform z = w x_2j + i w x_2j+1 (the
// pairing is by the frame's parity in the row, and a tile is even, so no tile splits a pair); a last odd frame has a zero
// partner.  Per pair: the two reflected, windowed frames into z[N], forward<N>, and for k <= N / 2, with Z[N] = Z[0],
//   A = 0.5 ((Z.re[k] + Z.re[N - k]), (Z.im[k] - Z.im[N - k])),   B = 0.5 ((Z.im[k] + Z.im[N - k]), (Z.re[N - k] - Z.re[k]))
// then by the kind of output:
//   complex       re into line k, im into line K + k of the tile                                      lines = 2 K
//   power 1 or 2  P = fma(re, re, round(im im)), its root for power 1, the log, into line k         lines = K
//   filterbank    the two frames' P or root into v[2][K] in LDS, a barrier, then line m is the chain fma(w[i], v[first_m + i],
//                 acc) over its band from zero, the log, into line m of the tile: only lines x tile is held, not K x tile
// and behind the last pair the tile's lines go to global memory, neighbouring lanes neighbouring frames.
//
// LDS: z, 8 N bytes; the tile [lines][tile + 1] floats -- the unpacking writes a column, neighbouring lanes neighbouring
// lines, and ds_write_b32 banks modulo 32 within 32 lanes, so the odd stride tile + 1 keeps it free of conflicts, and the
// store reads along a line --; with a filterbank v, 8 K bytes.
// The tile: alac_stft_cap(N) = 32768 / N frames, at most 64 (16 at 2048, 32 at 1024, 64 below) -- more would leave a batch of
// one-second rows too few workgroups --, halved once where that brings the workgroup from above to at or below 80 KiB, half
// of a CU's 160 KiB, so that two workgroups share a CU.  Power at 2048: 16 KiB + 1025 x 17 x 4 = 84.1 KiB at 16 frames,
// 16 + 1025 x 9 x 4 = 52.0 KiB at 8: 8.  Complex at 2048: 16 + 2050 x 17 x 4 = 152.1 KiB at 16, 88.1 KiB at 8, one workgroup
// either way: 16.  128 mel lines at 2048: 16 + 8 + 128 x 17 x 4 = 32.5 KiB: 16.  Every other shape is at or below 80 KiB.
// No scratch, no atomics, every element has one writer, all loads and stores are plain vector ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alac_fft_tile.h"

constexpr uint32_t ALAC_STFT_MAX_LINES = 256u;          // the lines of a filterbank
constexpr size_t ALAC_STFT_LDS_DEFAULT = 64u << 10;     // what a launch may ask for without an attribute
constexpr size_t ALAC_STFT_LDS_SHARE = 80u << 10;       // half a CU's LDS
constexpr size_t ALAC_STFT_LDS_MAX = 160u << 10;

enum { ALAC_STFT_COMPLEX = 0, ALAC_STFT_MAGNITUDE = 1, ALAC_STFT_POWER = 2 };
enum { ALAC_STFT_LOG_NONE = 0, ALAC_STFT_LOG_LN = 1, ALAC_STFT_LOG_10 = 2 };

__host__ __device__ constexpr bool alac_stft_n_fft_ok(uint32_t n) { return n == 256u || n == 512u || n == 1024u || n == 2048u; }
// the lines of the output: the filterbank's, or K, or 2 K for the complex spectrum
__host__ __device__ constexpr uint32_t alac_stft_lines(uint32_t n_fft, int power, uint32_t fb_lines) {
    return fb_lines ? fb_lines : (power == ALAC_STFT_COMPLEX ? n_fft + 2u : n_fft / 2u + 1u);
}
__host__ __device__ constexpr uint32_t alac_stft_cap(uint32_t n_fft) { return 32768u / n_fft < 64u ? 32768u / n_fft : 64u; }
// the bytes of LDS of a workgroup with a tile of `tile` frames: z, the tile and v
__host__ __device__ constexpr size_t alac_stft_lds_bytes(uint32_t n_fft, uint32_t lines, bool fb, uint32_t tile) {
    return 8u * (size_t)n_fft + 4u * (size_t)lines * (tile + 1u) + (fb ? 8u * (size_t)(n_fft / 2u + 1u) : 0u);
}
__host__ __device__ constexpr uint32_t alac_stft_tile(uint32_t n_fft, uint32_t lines, bool fb) {
    const uint32_t cap = alac_stft_cap(n_fft);
    return alac_stft_lds_bytes(n_fft, lines, fb, cap) > ALAC_STFT_LDS_SHARE && alac_stft_lds_bytes(n_fft, lines, fb, cap / 2u) <= ALAC_STFT_LDS_SHARE
               ? cap / 2u : cap;
}

struct alac_stft_params {
    const float* src;             // [planes, src_stride]
    uint64_t src_stride;
    uint64_t frames;              // the samples of a plane that are signal: L >= n_fft / 2 + 1
    float* out;                   // [planes, lines, out_frames]
    uint64_t out_frames;          // 1 + frames / hop
    const float* window;          // [n_fft]: the window at its offset, zeros around it
    const float2* table;          // [n_fft]: exp(-2 pi i k / n_fft)
    const uint32_t* bands;        // [fb_lines][3]: (first, count) of a line's band and where its weights begin, or null
    const float* weights;         // the bands' weights, packed in the order of the lines
    uint32_t hop, lines, fb_lines;
    uint32_t tile;                // alac_stft_tile
    uint32_t tiles;               // ceil(out_frames / tile): blockIdx.x = plane * tiles + tile index
    uint32_t power;               // ALAC_STFT_COMPLEX, _MAGNITUDE or _POWER
    uint32_t log_mode;
    float floor;
};

template <uint32_t N> __global__ void alac_stft_kernel(alac_stft_params p);
// the kernel of n_fft, for the host
const void* alac_stft_kernel_of(uint32_t n_fft);
