// alac_biquad.h -- the launch parameters and the blocking of the biquad cascade on the waveform (alac_biquad.hip), shared with
// the C ABI (alacgpu_stages.hip).  The signal is planar float32 [rows, channels, stride], the first `frames` of a plane are
// data; the coefficients are float64 [rows, sections, 5] = (b0, b1, b2, a1, a2), the gains float64 [rows].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A workgroup of ALAC_BIQUAD_THREADS lanes takes one (row, channel) and walks it in tiles of ALAC_BIQUAD_TILE frames in
// ascending order; lane l of a tile owns the ALAC_BIQUAD_CHUNK consecutive frames from ALAC_BIQUAD_CHUNK * l on, as float64 in
// registers, through all sections.  Per section a lane runs the FIR part and the zero-state recursion over its chunk; the
// chunk-end states (y[n-1], y[n-2]) are combined by a scan with the powers of M, the section's transition matrix over a
// chunk: ALAC_BIQUAD_LEVELS steps within a wave of 64 lanes (P_i = M^(2^i), i = 0 .. 5), then wave after wave with P_6, the
// state behind the last wave being carried to the next tile.  The state in front of lane l of wave w is then M^l c_w (the
// product of the P_i of l's set bits, ascending) plus the scan's value of the lane below, and the lane adds it through the two
// homogeneous responses h1, h2 of the section over a chunk.  h1, h2 and the P_i are computed once per row and section by
// running the recurrence over a chunk and by squaring M -- the squares are then powers of one and the same matrix, which on a
// narrow low filter keeps the scan ten times closer to the sequential evaluation than P_i taken from the recurrence run over
// 64 chunks -- into LDS (ALAC_BIQUAD_TAB doubles a section).  alac.net_amd/biquad.py states every
// operation in order; its twin follows them.  The tile is read into registers before it is written and nothing behind it is
// read again, so d_out may be d_src.
constexpr int ALAC_BIQUAD_THREADS = 256;
constexpr uint32_t ALAC_BIQUAD_CHUNK = 16u;
constexpr uint32_t ALAC_BIQUAD_TILE = 4096u;
static_assert(ALAC_BIQUAD_TILE == ALAC_BIQUAD_CHUNK * ALAC_BIQUAD_THREADS, "a tile is a chunk per lane");
constexpr uint32_t ALAC_BIQUAD_LEVELS = 6u;                     // 2^6 lanes a wave
constexpr uint32_t ALAC_BIQUAD_MAX_SECTIONS = 8u;
// a section's table: the 5 coefficients, h1 and h2 over a chunk, P_0 .. P_6 as (p00, p01, p10, p11); an even count
constexpr uint32_t ALAC_BIQUAD_TAB_H = 5u, ALAC_BIQUAD_TAB_P = ALAC_BIQUAD_TAB_H + 2u * ALAC_BIQUAD_CHUNK;
constexpr uint32_t ALAC_BIQUAD_TAB = (ALAC_BIQUAD_TAB_P + 4u * (ALAC_BIQUAD_LEVELS + 1u) + 1u) & ~1u;

struct alac_biquad_params {
    const float* src;             // [rows * channels, stride]
    float* out;                   // the same layout; may be src
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), frames), null: frames
    const double* coeffs;         // [rows, sections, 5]
    const double* gain;           // [rows] or null: 1
    uint32_t channels, sections;
    uint64_t stride, frames;
    uint32_t clamp;               // 0 / 1
    uint32_t vec;                 // 16-byte loads and stores: both bases and the stride are multiples of 16 bytes
};

__global__ void alac_biquad_kernel(alac_biquad_params p);
