// alac_fbank.h -- the launch parameters of the fused Kaldi fbank kernel (alac_fbank.hip), shared with the C ABI
// (alacgpu_stages.hip).  The tile, block, round and skew constants are the log-mel kernel's (alac_features.h).
#pragma once
#include "alac_features.h"

constexpr uint32_t ALAC_FBANK_MIN_WIN = 16u;
constexpr uint32_t ALAC_FBANK_MAX_WIN = 2048u;
constexpr uint32_t ALAC_FBANK_MAX_NFFT = 2048u;
constexpr uint32_t ALAC_FBANK_MEAN_PARTIALS = 8u;       // partial sums of a frame's mean: ALAC_FEATURES_THREADS / ALAC_FEATURES_TILE
constexpr float ALAC_FBANK_FLOOR = 1.1920928955078125e-07f;   // 2^-23, FLT_EPSILON

enum { ALAC_FBANK_SNIP_EDGES = 1, ALAC_FBANK_REMOVE_DC = 2, ALAC_FBANK_USE_POWER = 4, ALAC_FBANK_LOG = 8, ALAC_FBANK_FLAGS = 15 };

// The frames of a row of `frames` samples.  snip_edges: whole windows only; else one frame per hop, centred.
__host__ __device__ inline uint64_t alac_fbank_frames(uint64_t frames, uint32_t win, uint32_t hop, bool snip_edges) {
    if (snip_edges) return frames < win ? 0u : 1u + (frames - win) / hop;
    return (frames + hop / 2u) / hop;
}

// LDS: the window, the mel sums, the power of a round of bin blocks, the means of the tile's frames, the skewed span -- the
// log-mel kernel's layout with a window of win taps, the bins of n_fft and the means
struct alac_fbank_lds {
    uint32_t window, mel, power, mean, span;   // floats of each part, in this order
    __host__ __device__ size_t bytes() const { return sizeof(float) * ((size_t)window + mel + power + mean + span); }
};

__host__ __device__ inline alac_fbank_lds alac_fbank_lds_layout(uint32_t win, uint32_t n_fft, uint32_t hop, uint32_t n_mels) {
    const uint32_t n_bins = n_fft / 2u + 1u;
    const uint32_t blocks = (n_bins + ALAC_FEATURES_BLOCK - 1u) / ALAC_FEATURES_BLOCK;
    const uint32_t span = (alac_features_tile(win, hop) - 1u) * hop + win;
    alac_fbank_lds l;
    l.window = (win + 3u) & ~3u;
    l.mel = n_mels * ALAC_FEATURES_TILE;
    l.power = (blocks < ALAC_FEATURES_ROUND_BLOCKS ? blocks : ALAC_FEATURES_ROUND_BLOCKS) * ALAC_FEATURES_BLOCK * ALAC_FEATURES_TILE;
    l.mean = ALAC_FEATURES_TILE;
    l.span = span + alac_features_skew(hop) * ((span - 1u) / hop + 1u);
    return l;
}

struct alac_fbank_params {
    const float* src;             // [planes, src_stride]
    uint64_t src_stride;
    uint64_t frames;              // the samples of a plane that are signal: L >= 1
    float* out;                   // [planes, n_mels, out_frames]
    uint64_t out_frames;          // alac_fbank_frames(frames, win, hop, snip_edges) >= 1
    const float* window;          // [win]
    const float* basis;           // [win, 2 * n_bins]
    const float* fb;              // [n_mels, n_bins]
    uint32_t win, n_fft, hop, n_mels;
    uint32_t tile;                // alac_features_tile(win, hop)
    uint32_t tiles;               // ceil(out_frames / tile): blockIdx.x = plane * tiles + tile index
    uint32_t flags;               // ALAC_FBANK_*
    float preemphasis, scale;
};

__global__ void alac_fbank_kernel(alac_fbank_params p);
