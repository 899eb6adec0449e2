// alac_fbank.h -- the launch parameters of the fused Kaldi fbank kernel (alac_fbank.hip), shared with the C ABI
// (alacgpu_stages.hip).  The shared launch fields, the LDS layout, the constants and the tile body are alac_features.h's.
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

constexpr uint32_t ALAC_FBANK_LDS_EXTRA = ALAC_FEATURES_TILE;  // the kernel's own part of alac_features_lds_layout: the means of the tile's frames

struct alac_fbank_params : alac_stft_mel_params {   // taps: win; frames: L >= 1; out_frames: alac_fbank_frames(...) >= 1
    uint32_t flags;               // ALAC_FBANK_*
    float preemphasis, scale;
};

__global__ void alac_fbank_kernel(alac_fbank_params p);
