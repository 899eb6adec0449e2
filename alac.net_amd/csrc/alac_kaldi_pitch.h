// alac_kaldi_pitch.h -- the launch parameters, the packed tables and the scratch layout of Kaldi's pitch features
// (alac_kaldi_pitch.hip), shared with the C ABI (alacgpu_stages.hip).  Three launches: the downsampled rows with the partial sums
// of their mean square, the NCCF of every frame on the lag grid (a wave per frame), the dense Viterbi decode along every plane
// with the post-processing as its epilogue.  alac.net_amd/kaldi_pitch.py states every operation in order; its float32 twin
// follows them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t ALAC_KPITCH_MAX_STATES = 1024u, ALAC_KPITCH_MAX_DOWN = 4096u, ALAC_KPITCH_MAX_LDS = 65536u;
constexpr uint32_t ALAC_KPITCH_CHUNK = 1024u, ALAC_KPITCH_HEAD = 8u;
constexpr int ALAC_KPITCH_THREADS = 256, ALAC_KPITCH_DECODE_THREADS = 512;
constexpr uint32_t ALAC_KPITCH_PROCESS = 1u, ALAC_KPITCH_POV = 2u, ALAC_KPITCH_NORM = 4u, ALAC_KPITCH_DELTA = 8u, ALAC_KPITCH_RAW = 16u;

// The framing of a specification (kaldi_pitch.KaldiPitch): the input's rate, frame length and shift, and those at resample_freq
struct alac_kpitch_framing {
    uint32_t sample_rate, resample_freq, win_in, hop_in, window, shift;
};

// N(v): the downsampled samples of a row of v samples
__host__ __device__ inline uint64_t alac_kpitch_samples(const alac_kpitch_framing& f, uint64_t v) {
    return (v * f.resample_freq + f.sample_rate - 1u) / f.sample_rate;
}

// frames(v): the smaller of KaldiFbank's count and Kaldi's own
__host__ __device__ inline uint64_t alac_kpitch_frames(const alac_kpitch_framing& f, uint64_t v) {
    const uint64_t n = alac_kpitch_samples(f, v);
    const uint64_t a = v < f.win_in ? 0u : 1u + (v - f.win_in) / f.hop_in;
    const uint64_t k = n < f.window ? 0u : 1u + (n - f.window) / f.shift;
    return a < k ? a : k;
}

__host__ __device__ inline uint32_t alac_kpitch_lines(uint32_t flags) {
    if (!(flags & ALAC_KPITCH_PROCESS)) return 2u;
    return ((flags >> 1) & 1u) + ((flags >> 2) & 1u) + ((flags >> 3) & 1u) + ((flags >> 4) & 1u);
}

// The float32 tables of a specification, packed in this order (kaldi_pitch.KaldiPitch.table): the head [8] (the transition's
// factor, the pre-emphasis, nccf_ballast, pitch_scale, pov_scale, pov_offset, delta_pitch_scale, 0), the downsampler's first
// input index per phase [phases] (integers as floats) and its weights [phases, down_taps], the interpolation's first lag index
// per state [n_states] and its weights [n_states, up_taps], soft_min_f0 * lag [n_states], 1 / lag in Hz [n_states], the delta's
// coefficients [2 delta_window + 1]
struct alac_kpitch_tables {
    const float *head, *down_first, *down, *up_first, *up, *sl, *hz, *dc;
};

inline alac_kpitch_tables alac_kpitch_tables_at(const float* t, uint32_t phases, uint32_t down_taps, uint32_t n_states, uint32_t up_taps) {
    alac_kpitch_tables a;
    a.head = t;
    a.down_first = a.head + ALAC_KPITCH_HEAD;
    a.down = a.down_first + phases;
    a.up_first = a.down + (size_t)phases * down_taps;
    a.up = a.up_first + n_states;
    a.sl = a.up + (size_t)n_states * up_taps;
    a.hz = a.sl + n_states;
    a.dc = a.hz + n_states;
    return a;
}

// What a call keeps in the ctx's scratch, buf[0]: the partial sums (double2 [planes, chunks]) in front, the downsampled rows
// (float [planes, n_max]), the NCCF planes (float [planes, 2, out_frames, n_states]: stage 0 only), the raw track and the
// epilogue's weights and log-pitches (float [planes, 2, out_frames] each).  buf[1]: the uint16 backpointers
// [planes, out_frames, n_states].
struct alac_kpitch_scratch {
    uint64_t sums, down, nccf, raw, work, bytes0, bytes1;     // byte offsets into buf[0]; the two sizes
};

inline alac_kpitch_scratch alac_kpitch_scratch_of(uint64_t planes, uint64_t n_max, uint64_t out_frames, uint32_t n_states, bool down,
                                                   bool nccf, bool decode, bool lines) {
    alac_kpitch_scratch s;
    const uint64_t chunks = (n_max + ALAC_KPITCH_CHUNK - 1u) / ALAC_KPITCH_CHUNK;
    s.sums = 0u;
    s.down = s.sums + (down ? 16u * planes * chunks : 0u);
    s.nccf = s.down + (down ? 4u * planes * n_max : 0u);
    s.raw = s.nccf + (nccf ? 8u * planes * out_frames * n_states : 0u);
    s.work = s.raw + (lines ? 8u * planes * out_frames : 0u);
    s.bytes0 = s.work + (lines ? 8u * planes * out_frames : 0u);
    s.bytes1 = decode ? 2u * planes * out_frames * n_states : 0u;
    return s;
}

// The first launch: a workgroup per chunk of ALAC_KPITCH_CHUNK downsampled samples of a plane
struct alac_kpitch_down_params {
    const float* src;             // [rows, channels, stride]
    const int64_t* valid;         // [rows] or null
    float* down;                  // [planes, n_max]
    double* sums;                 // [planes, chunks, 2]: the chunk's sum and sum of squares
    alac_kpitch_tables tab;
    alac_kpitch_framing fr;
    uint32_t channels, phases, in_per_unit, down_taps, chunks;
    uint64_t stride, frames, n_max;
};

// The second: a wave per frame, ALAC_KPITCH_THREADS / 64 frames per workgroup.  LDS per wave: the frame's span + 2 n_lags floats.
struct alac_kpitch_nccf_params {
    const int64_t* valid;
    const float* down;            // [planes, n_max]
    const double* sums;           // [planes, chunks, 2]
    float* nccf;                  // [planes, 2, out_frames, n_states]
    alac_kpitch_tables tab;
    alac_kpitch_framing fr;
    uint32_t channels, chunks, first_lag, last_lag, n_states, up_taps, groups;   // groups: workgroups per plane
    uint64_t frames, n_max, out_frames;
};

inline size_t alac_kpitch_nccf_lds(uint32_t window, uint32_t first_lag, uint32_t last_lag) {
    return sizeof(float) * (size_t)(ALAC_KPITCH_THREADS / 64) * ((size_t)window + last_lag + 2u * (last_lag - first_lag + 1u));
}

// The third: one workgroup of ALAC_KPITCH_DECODE_THREADS lanes per plane, sequential over that plane's frames.  The forward
// costs are double-buffered in LDS; a lane takes the targets tid, tid + 512; the backpointers are uint16 source states.  One lane
// walks back and leaves the raw track; the post-processing is the epilogue, a lane per frame.
struct alac_kpitch_decode_params {
    const float* nccf;            // [planes, 2, out_frames, n_states] or null (stage 3: the raw track is given)
    const int64_t* valid;         // [rows] or null: samples of a row, or with counts_are_frames its frames
    uint16_t* back;               // [planes, out_frames, n_states]
    float* raw;                   // [planes, 2, out_frames]: written by the walk back, or given
    float* work;                  // [planes, 2, out_frames] or null (no post-processing)
    float* out;                   // [planes, lines, out_frames] or null
    alac_kpitch_tables tab;
    alac_kpitch_framing fr;
    uint32_t channels, n_states, flags, left, right, delta_window, counts_are_frames;
    uint64_t frames, out_frames;
};

__global__ void alac_kpitch_down_kernel(alac_kpitch_down_params p);
__global__ void alac_kpitch_nccf_kernel(alac_kpitch_nccf_params p);
__global__ void alac_kpitch_decode_kernel(alac_kpitch_decode_params p);
