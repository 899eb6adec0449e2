// alac_level.h -- the launch parameters, the blocking and the order of the sums of the level stage on the waveform
// (alac_level.hip), shared with the C ABI (alacgpu_stages.hip).  The signal is planar float32 [rows, channels, stride], the
// first `frames` of a plane are data.  Two launches: alac_level_measure_kernel fills the scratch, alac_level_apply_kernel
// combines it into the row's gain and writes g x.  include/alacgpu.h states the arithmetic, alac.net_amd/level.py every
// operation in order; its twin follows them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alac_biquad.h"

constexpr uint32_t ALAC_LEVEL_PEAK = 0u;
constexpr uint32_t ALAC_LEVEL_RMS = 1u;
constexpr uint32_t ALAC_LEVEL_LUFS = 2u;
constexpr int ALAC_LEVEL_THREADS = 256;
constexpr uint32_t ALAC_LEVEL_MAX_CHANNELS = 5u;     // BS.1770's weights: L, R, C, Ls, Rs (lufs only)
constexpr uint32_t ALAC_LEVEL_MIN_HOP = 16u;         // a chunk of ALAC_BIQUAD_CHUNK frames then touches at most two hops
static_assert(ALAC_LEVEL_MIN_HOP >= ALAC_BIQUAD_CHUNK && ALAC_LEVEL_THREADS == ALAC_BIQUAD_THREADS, "the measure launch walks the biquad's tiles");
constexpr uint32_t ALAC_LEVEL_HEAD = 2u;             // the scratch of a plane: the sum of squares, the peak, then the hop sums
// BS.1770: the channel weights, and the absolute gate 10^((-70 + 0.691) / 10) as the double nearest to it (level.py holds the
// same literal: a power is not correctly rounded, so neither the kernel nor the entry evaluates one)
constexpr double ALAC_LEVEL_WEIGHT_FRONT = 1.0, ALAC_LEVEL_WEIGHT_SURROUND = 1.41;
constexpr double ALAC_LEVEL_GATE_ABS = 1.1724653045822981e-07;
constexpr double ALAC_LEVEL_GATE_REL = 0.1;
// the apply launch: a row is cut into parts of ALAC_LEVEL_PART frames, the smallest multiple of it that keeps a row within
// ALAC_LEVEL_MAX_PARTS parts; a workgroup takes one part of every channel of its row
constexpr uint32_t ALAC_LEVEL_PART = 4096u;
constexpr uint32_t ALAC_LEVEL_MAX_PARTS = 256u;
constexpr uint32_t ALAC_LEVEL_BATCH = 256u;          // blocks whose energies a workgroup evaluates side by side (the order of their sum does not depend on it)

inline uint64_t alac_level_part_frames(uint64_t frames) {
    const uint64_t least = (frames + ALAC_LEVEL_PART - 1u) / ALAC_LEVEL_PART;
    const uint64_t k = (least + ALAC_LEVEL_MAX_PARTS - 1u) / ALAC_LEVEL_MAX_PARTS;
    return (uint64_t)ALAC_LEVEL_PART * (k ? k : 1u);
}
inline uint32_t alac_level_parts(uint64_t frames) {
    const uint64_t pf = alac_level_part_frames(frames);
    return (uint32_t)((frames + pf - 1u) / pf);
}
// the hop sums a plane of `frames` frames can have, and the doubles of its scratch
inline uint64_t alac_level_hops(uint32_t mode, uint64_t frames, uint32_t hop) { return mode == ALAC_LEVEL_LUFS ? frames / hop : 0u; }

// The order of the sums (v the row's valid frames, every operation one IEEE float64 operation, none fused):
//   measure, one workgroup per (row, channel), tiles of ALAC_BIQUAD_TILE frames in ascending order, lane l of a tile the chunk
//   of ALAC_BIQUAD_CHUNK frames from 16 l on (a frame at or behind v is not read and counts as 0):
//     the sum of squares: the lane's 16 squares of x (exact in float64) added in ascending order from 0; the 64 lanes of a wave
//       as a tree of halves (q[l] += q[l + h], h = 32 .. 1), the 4 waves likewise (h = 2, 1), the tiles in ascending order
//     the peak: the largest |x|, a NaN if there is one
//     lufs: the chunk through the two K-weighting sections by the biquad's tile body; nh = v / hop whole hops count, frames at
//       or behind nh hop belong to none.  A chunk touches at most two hops: its squares (rounded once) are added in ascending
//       order from 0 into one partial per hop it touches.  s[k] is the sum of the partials of hop k in ascending order of their
//       chunks, from 0 -- whatever tile a chunk lies in, so a chunk that straddles a hop boundary gives its first frames to
//       the end of one sum and its last frames to the beginning of the next
//   apply, every workgroup of a row for itself:
//     P = the largest peak of the channels; S = the channels' sums of squares added in ascending order from S_0
//     peak: g = target / P;  rms: E = S / (channels v), g = sqrt(target / E)
//     lufs: for block j < nh - 3: z_c = ((s_c[j] + s_c[j+1]) + (s_c[j+2] + s_c[j+3])) / (4 hop), e[j] = G_0 z_0, then + G_c z_c
//       in ascending order; m1 = (the sum of the e[j] > Gabs in ascending order from 0) / their count; E = (the sum of the
//       e[j] > Gabs that are also > 0.1 m1, in ascending order from 0) / their count; g = sqrt(target / E)
//     max_peak > 0: m = max_peak / P, g = m where m < g
//     y = fl32(g * x), x widened exactly, rounded once; with clamp then min(max(y, -1), 1), a NaN kept
//   A row with v == 0, P == 0, E == 0, or for lufs nh < 4 or no e[j] above Gabs, has g = 1 and is not written; nor is a row
//   whose g is exactly 1 without clamp.
struct alac_level_params {
    const float* src;             // [rows * channels, stride]
    float* out;                   // the same layout; may be src; null: measure only
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), frames), null: frames
    const double* kweight;        // [2, 5]: the two K-weighting sections (lufs)
    double* scratch;              // [rows, channels, ALAC_LEVEL_HEAD + hops]
    double* gain_out;             // [rows] or null
    double* energy_out;           // [rows] or null
    double* peak_out;             // [rows] or null
    double target, max_peak;      // linear; max_peak <= 0: none
    uint64_t stride, frames, hops, part_frames;
    uint32_t channels, mode, hop, parts;
    uint32_t clamp;               // 0 / 1
    uint32_t vec;                 // the measure launch's 16-byte loads: src and the stride are multiples of 16 bytes
    uint32_t vec_out;             // the apply launch's 16-byte loads and stores: out is one too
};

__global__ void alac_level_measure_kernel(alac_level_params p);
__global__ void alac_level_apply_kernel(alac_level_params p);
