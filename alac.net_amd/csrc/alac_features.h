// alac_features.h -- the launch parameters of the fused STFT + mel + log kernel (alac_features.hip), shared with the C ABI
// (alacgpu_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ALAC_FEATURES_THREADS = 256;
constexpr uint32_t ALAC_FEATURES_TILE = 32u;            // frames of a tile: the N of v_mfma_f32_32x32x2_f32
constexpr uint32_t ALAC_FEATURES_BLOCK = 32u;           // bins of a block: its M
constexpr uint32_t ALAC_FEATURES_ROUND_BLOCKS = 8u;     // bin blocks whose power is in LDS at a time (two per wave)
constexpr uint32_t ALAC_FEATURES_MIN_NFFT = 16u;
constexpr uint32_t ALAC_FEATURES_MAX_NFFT = 2048u;
constexpr uint32_t ALAC_FEATURES_MAX_MELS = 256u;
constexpr uint32_t ALAC_FEATURES_MAX_SPAN = 19456u;     // samples of a tile's span: 76 KiB of LDS (+ 4 KiB of skew at most)
constexpr size_t ALAC_FEATURES_LDS_DEFAULT = 64u << 10; // what a launch may ask for without an attribute
constexpr size_t ALAC_FEATURES_LDS_MAX = 160u << 10;    // what a CU has

// The frames a workgroup takes: ALAC_FEATURES_TILE, fewer only where the span of that many, (tile - 1) hop + n_fft samples,
// is more than ALAC_FEATURES_MAX_SPAN (hop above 561 at n_fft 2048); one frame's span, n_fft, always fits.
__host__ __device__ inline uint32_t alac_features_tile(uint32_t n_fft, uint32_t hop) {
    if ((ALAC_FEATURES_TILE - 1u) * hop + n_fft <= ALAC_FEATURES_MAX_SPAN) return ALAC_FEATURES_TILE;
    return 1u + (ALAC_FEATURES_MAX_SPAN - n_fft) / hop;
}

// The span in LDS: sample i of it lives at i + skew * (i / hop).  The lanes of a wave read the same tap of 32 neighbouring
// frames, hop samples apart: with an even hop (160: every lane in one of two banks) one float of padding per hop makes the
// stride odd and the 32 addresses fall into 32 banks.
__host__ __device__ inline uint32_t alac_features_skew(uint32_t hop) { return (hop & 1u) ? 0u : 1u; }

struct alac_features_lds {
    uint32_t window, mel, power, span;   // floats of each part, in this order
    __host__ __device__ size_t bytes() const { return sizeof(float) * ((size_t)window + mel + power + span); }
};

__host__ __device__ inline alac_features_lds alac_features_lds_layout(uint32_t n_fft, uint32_t hop, uint32_t n_mels) {
    const uint32_t n_bins = n_fft / 2u + 1u;
    const uint32_t blocks = (n_bins + ALAC_FEATURES_BLOCK - 1u) / ALAC_FEATURES_BLOCK;
    const uint32_t span = (alac_features_tile(n_fft, hop) - 1u) * hop + n_fft;
    alac_features_lds l;
    l.window = (n_fft + 3u) & ~3u;
    l.mel = n_mels * ALAC_FEATURES_TILE;
    l.power = (blocks < ALAC_FEATURES_ROUND_BLOCKS ? blocks : ALAC_FEATURES_ROUND_BLOCKS) * ALAC_FEATURES_BLOCK * ALAC_FEATURES_TILE;
    l.span = span + alac_features_skew(hop) * ((span - 1u) / hop + 1u);
    return l;
}

enum { ALAC_FEATURES_LOG_NONE = 0, ALAC_FEATURES_LOG_LN = 1, ALAC_FEATURES_LOG_10 = 2 };

struct alac_features_params {
    const float* src;             // [planes, src_stride]
    uint64_t src_stride;
    uint64_t frames;              // the samples of a plane that are signal: L > n_fft / 2
    float* out;                   // [planes, n_mels, out_frames]
    uint64_t out_frames;          // 1 + frames / hop
    const float* window;          // [n_fft]
    const float* basis;           // [n_fft, 2 * n_bins]
    const float* fb;              // [n_mels, n_bins]
    uint32_t n_fft, hop, n_mels;
    uint32_t tile;                // alac_features_tile(n_fft, hop)
    uint32_t tiles;               // ceil(out_frames / tile): blockIdx.x = plane * tiles + tile index
    uint32_t log_mode;
    float floor;
};

__global__ void alac_logmel_kernel(alac_features_params p);
