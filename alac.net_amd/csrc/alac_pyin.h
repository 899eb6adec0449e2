// alac_pyin.h -- the launch parameters, the tables and the LDS images of the pYIN kernels (alac_pyin.hip), shared with the C ABI
// (alacgpu_stages.hip).  Two launches: the observation of every frame (the YIN tile of alac_yin.h for the difference function
// and d', then a wave per frame for the troughs and their probabilities) and the Viterbi decode along every plane.
// alac.net_amd/pyin.py states every operation in order; its float32 twin follows them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alac_yin.h"

constexpr uint32_t ALAC_PYIN_MAX_BINS = 1024u, ALAC_PYIN_MAX_THRESHOLDS = 256u;
constexpr int ALAC_PYIN_DECODE_THREADS = 256;
constexpr uint32_t ALAC_PYIN_LANE_THRESHOLDS = ALAC_PYIN_MAX_THRESHOLDS / 64u;      // threshold i belongs to lane (i - 1) % 64

// The most troughs a frame has: no two are neighbours (pyin.PYin.max_troughs)
inline uint32_t alac_pyin_max_troughs(uint32_t tau_min, uint32_t tau_max) { return (tau_max - tau_min + 1u) / 2u; }

// The float32 tables of a specification, packed in this order (pyin.PYin.table): the thresholds s [N], their Beta weights [N],
// the weights' sums cb [N + 1], the Boltzmann factors bz [K + 1] and truncations inv [K + 1] (K the most troughs), the period
// edges [n_bins - 1], descending, the bin frequencies [n_bins], lz [n_bins], lt [band + 1], ls [2] (stay, switch), lstart [1]
struct alac_pyin_tables {
    const float *s, *beta, *cb, *bz, *inv, *edges, *freq, *lz, *lt, *ls, *lstart;
};

inline alac_pyin_tables alac_pyin_tables_at(const float* t, uint32_t N, uint32_t K, uint32_t n_bins, uint32_t band) {
    alac_pyin_tables a;
    a.s = t;
    a.beta = a.s + N;
    a.cb = a.beta + N;
    a.bz = a.cb + N + 1u;
    a.inv = a.bz + K + 1u;
    a.edges = a.inv + K + 1u;
    a.freq = a.edges + n_bins - 1u;
    a.lz = a.freq + n_bins;
    a.lt = a.lz + n_bins;
    a.ls = a.lt + band + 1u;
    a.lstart = a.ls + 2u;
    return a;
}

// The observation: the grid, the tile and the front of the LDS image are alac_yin_kernel's (y; y.out is not used).  Behind the
// difference functions of a whole tile lie bz and inv, [K + 1] floats each, and one line of n_bins probabilities per wave.
struct alac_pyin_obs_params {
    alac_yin_params y;
    alac_pyin_tables tab;
    float* obs_voiced;            // [rows * channels, out_frames, n_bins]: log2 observations of the voiced states
    float* obs_unvoiced;          // [rows * channels, out_frames]: of every unvoiced state
    float* vp;                    // [rows * channels, out_frames]: the voicing probability
    uint32_t n_thresholds, n_bins, max_troughs;
    float no_trough;
};

inline size_t alac_pyin_obs_lds_floats(const alac_yin_params& y, uint32_t K, uint32_t n_bins) {
    return (size_t)y.samples + (size_t)y.tile * (y.tau_max + 1u) + 2u * (K + 1u) + (size_t)(ALAC_YIN_THREADS / 64) * n_bins;
}

// The decode: one workgroup of ALAC_PYIN_DECODE_THREADS lanes per plane, sequential over that plane's frames.  e = delta - lz
// of both halves is double-buffered in LDS (2 * 2 * 1024 floats), the last delta beside it for the final arg-max; a lane takes
// the targets tid, tid + 256, .. of both halves, so one __syncthreads a frame.  The backpointers are uint16 source states
// [planes, out_frames, 2 n_bins].  One lane walks back and stores the lines.
struct alac_pyin_decode_params {
    const float* obs_voiced;      // [planes, out_frames, n_bins]
    const float* obs_unvoiced;    // [planes, out_frames]
    const float* vp;              // [planes, out_frames] or null (no line 2: the states alone are asked for)
    const int64_t* valid;         // [rows] or null: samples of a row (frames by y's framing) or, with counts_are_frames, its frames
    uint16_t* back;               // [planes, out_frames, 2 n_bins]
    float* out;                   // [planes, 3, out_frames] or null
    int32_t* states;              // [planes, out_frames] or null: the path, -1 at and behind the count
    alac_pyin_tables tab;
    uint32_t channels, n_bins, band;
    uint64_t frames, out_frames;  // the samples of a plane (unused with counts_are_frames), the frames of a line
    uint32_t hop, align;
    uint32_t counts_are_frames;
};

__global__ void alac_pyin_obs_kernel(alac_pyin_obs_params p);
__global__ void alac_pyin_obs_kernel_vec(alac_pyin_obs_params p);
__global__ void alac_pyin_decode_kernel(alac_pyin_decode_params p);
