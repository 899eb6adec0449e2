// alac_mix.h -- the launch parameters, the part size and the order of the sums of the noise mix between the crops and their
// features (alac_mix.hip), shared with the C ABI (alacgpu_stages.hip).  The data is float32, planar: the signal and the
// result [rows, channels, stride], the noise [rows, noise_channels, noise_stride] with noise_channels 1 or channels; the
// first `frames` elements of a plane are data.  include/alacgpu.h states the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A workgroup of ALAC_MIX_THREADS takes one part of a row: ALAC_MIX_PART consecutive frames of every channel, or the smallest
// multiple of that which keeps a row within ALAC_MIX_MAX_PARTS parts (rows of 2^20 frames and more).  A thread takes
// ALAC_MIX_VEC consecutive frames at a time -- one 16-byte load or store where the plane's base and stride are multiples of
// 16 bytes, ALAC_MIX_VEC 4-byte ones where they are not -- and a workgroup ALAC_MIX_ROUND = ALAC_MIX_THREADS * ALAC_MIX_VEC
// frames in a round.  A part begins at a multiple of ALAC_MIX_ROUND.
//
// The order of the float32 sums, which the twin in alac.net_amd/mix.py follows and which does not depend on the width of the
// loads.  Both sums of a row, of x[c, i]^2 over i < v and of n[c, i]^2 over i < vn, are taken part by part over the same
// parts of 0 .. frames.  Within the part that begins at frame f0, partial j of ALAC_MIX_ROUND is
//   ((0 + t[0, f0 + j]) + t[0, f0 + j + ROUND]) + t[0, f0 + j + 2 ROUND] ... then channel 1 likewise, and so on
// over the frames of the part below v (vn), t the squares, each rounded once.  The ALAC_MIX_VEC partials of a thread
// (j = VEC * thread + k) are added as a tree of halves, q[k] = q[k] + q[k + h] for h = 2, 1; the 64 sums of a wave by the same
// tree, h = 32 .. 1; the ALAC_MIX_THREADS / 64 wave sums by the same tree, h = 2, 1.  The parts of a row are then added in
// ascending order, ((0 + S[0]) + S[1]) + S[2] ...; a part without a frame below v (vn) is 0.
constexpr int ALAC_MIX_THREADS = 256;
constexpr uint32_t ALAC_MIX_VEC = 4u;
constexpr uint32_t ALAC_MIX_ROUND = 1024u;
constexpr uint32_t ALAC_MIX_PART = 4096u;
constexpr uint32_t ALAC_MIX_MAX_PARTS = 256u;
static_assert(ALAC_MIX_ROUND == ALAC_MIX_THREADS * ALAC_MIX_VEC && ALAC_MIX_PART % ALAC_MIX_ROUND == 0u && ALAC_MIX_VEC == 4u,
              "a thread takes a float4; a part is whole rounds");

__host__ __device__ inline uint64_t alac_mix_part_frames(uint64_t frames) {
    const uint64_t least = (frames + ALAC_MIX_PART - 1u) / ALAC_MIX_PART;                   // parts of ALAC_MIX_PART
    const uint64_t k = (least + ALAC_MIX_MAX_PARTS - 1u) / ALAC_MIX_MAX_PARTS;
    return (uint64_t)ALAC_MIX_PART * (k ? k : 1u);
}
__host__ __device__ inline uint32_t alac_mix_parts(uint64_t frames) {
    const uint64_t part = alac_mix_part_frames(frames);
    return (uint32_t)((frames + part - 1u) / part);
}

struct alac_mix_params {
    const float* src;             // [rows, channels, stride]
    float* out;                   // the same layout; may be src
    const float* noise;           // [rows, noise_channels, noise_stride]
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), frames), null: frames
    const int64_t* noise_valid;   // [rows] or null: vn likewise
    const float* ratio;           // [rows]: a
    float* sums;                  // [rows, parts, 2]: the sums of the squares of x and of n over a part; written by the reduce
                                  // launch, read by the apply launch
    uint32_t channels, noise_channels;
    uint64_t stride, noise_stride, frames;
    uint64_t part_frames;         // alac_mix_part_frames(frames)
    uint32_t parts;               // alac_mix_parts(frames): blockIdx.x = row * parts + part
    uint32_t vec, noise_vec;      // 16-byte loads and stores: src and out (both) / noise have base and stride at multiples of 16
};

__global__ void alac_mix_reduce_kernel(alac_mix_params p);
__global__ void alac_mix_apply_kernel(alac_mix_params p);
