// alac_mfcc.h -- the launch parameters of the fused Kaldi MFCC kernel (alac_mfcc.hip), shared with the C ABI
// (alacgpu_stages.hip).  The framing, its flags, the floor and the frame count are alac_fbank.h's; the shared launch fields,
// the LDS layout and the tile body are alac_features.h's.
#pragma once
#include "alac_fbank.h"

// alacgpu_mfcc_device's flags: fbank's 1, 2 and 4 (the log is not a choice), and the two of the energy
enum { ALAC_MFCC_USE_ENERGY = 16, ALAC_MFCC_RAW_ENERGY = 32,
       ALAC_MFCC_FLAGS = ALAC_FBANK_SNIP_EDGES | ALAC_FBANK_REMOVE_DC | ALAC_FBANK_USE_POWER | ALAC_MFCC_USE_ENERGY | ALAC_MFCC_RAW_ENERGY };

// the kernel's own part of alac_features_lds_layout: the means of the tile's frames, then their log energies
constexpr uint32_t ALAC_MFCC_LDS_EXTRA = 2u * ALAC_FEATURES_TILE;

struct alac_mfcc_params : alac_stft_mel_params {   // taps: win; n_mels: the filters; out: [planes, n_ceps, out_frames]
    const float* dct;             // [n_ceps, n_mels]
    const float* lifter;          // [n_ceps]
    uint32_t n_ceps;              // 1 .. n_mels
    uint32_t flags;               // ALAC_FBANK_SNIP_EDGES, _REMOVE_DC, _USE_POWER, ALAC_MFCC_*
    float preemphasis, scale;
    float log_energy_floor;       // ln(energy_floor) rounded once on the host; -infinity for energy_floor == 0
};

__global__ void alac_mfcc_kernel(alac_mfcc_params p);
