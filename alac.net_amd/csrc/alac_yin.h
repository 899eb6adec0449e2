// alac_yin.h -- the launch parameters and the tiling of the YIN pitch kernel (alac_yin.hip), shared with the C ABI
// (alacgpu_stages.hip).  The signal is planar float32 [rows, channels, stride], the first `frames` of a plane are data; the
// output is float32 [rows, channels, 2, out_frames]: f0 and the aperiodicity.  alac.net_amd/yin.py states every operation in
// order; its float32 twin follows them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A workgroup of ALAC_YIN_THREADS lanes takes one plane and a tile of consecutive frames, whose samples -- span + (tile - 1)
// * hop of them, consecutive frames overlap by span - hop -- it loads once into LDS, zeros outside the row's valid samples.
// Step 1, all of the arithmetic: an item is (frame of the tile, group of ALAC_YIN_LAGS consecutive lags); a lane takes items
// tid, tid + ALAC_YIN_THREADS, .. and slides along j four samples at a time, the lags' accumulators and a window of
// 2 * ALAC_YIN_LAGS - 1 samples in registers: two 16-byte LDS reads (the x[s + j] one a broadcast within a frame, the other
// consecutive across lanes) feed 16 subtractions and 16 fused multiply-adds.  Every lag's sum runs over j in ascending order in
// one lane, so neither the tile nor the mapping of items to lanes changes a bit.  The 16-byte reads need hop % 4 == 0 (every
// frame then starts on a 16-byte boundary of the LDS image); other hops read single floats, with the same result.  The
// difference functions go to LDS behind the samples, and one wave per frame does steps 2 to 5 out of it: the scan over the
// lags in chunks of 64 (six shuffle steps and a carry), the threshold search by ballots, the descent, the argmin by a
// lexicographic wave minimum, the parabola.
constexpr int ALAC_YIN_THREADS = 256;
constexpr uint32_t ALAC_YIN_LAGS = 4u;
constexpr uint32_t ALAC_YIN_MIN_WIN = 64u, ALAC_YIN_MAX_WIN = 2048u, ALAC_YIN_MAX_LAG = 2048u;
constexpr uint32_t ALAC_YIN_TILE_MAX = 8u;
constexpr uint32_t ALAC_YIN_LDS_FLOATS = 8192u;                  // 32 KiB: four workgroups a CU and more
constexpr uint32_t ALAC_YIN_PAD = 8u;                            // the window's reads behind the last lag, and the rounding to 16 bytes

// The frames of a tile: at most ALAC_YIN_TILE_MAX, fewer where their samples and difference functions would not fit
// (yin.tile_frames is this)
inline uint32_t alac_yin_tile(uint32_t win, uint32_t tau_max, uint64_t hop) {
    const uint64_t lags = tau_max + 1u, room = ALAC_YIN_LDS_FLOATS - ALAC_YIN_PAD - (win + tau_max) - lags;
    const uint64_t more = room / (hop + lags);
    return (uint32_t)(more + 1u < ALAC_YIN_TILE_MAX ? more + 1u : ALAC_YIN_TILE_MAX);
}

// The floats of the LDS image in front of the difference functions: the tile's samples and the window's overshoot, a
// multiple of 4
inline uint32_t alac_yin_samples(uint32_t win, uint32_t tau_max, uint64_t hop, uint32_t tile) {
    return (uint32_t)((win + tau_max + (tile - 1u) * hop + 4u + 3u) & ~(uint64_t)3u);
}

struct alac_yin_params {
    const float* src;             // [rows * channels, stride]
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), frames), null: frames
    float* out;                   // [rows * channels, 2, out_frames]
    uint32_t channels;
    uint64_t stride, frames, out_frames;
    uint32_t win, hop, tau_min, tau_max;
    uint32_t align;               // 0: centred frames, v / hop + 1 of them; else 1 + (v - align) / hop, none for v < align
    int64_t first;                // the first sample of frame 0 (negative: zeros are read)
    uint32_t tile, tiles;         // frames a workgroup, workgroups a plane
    uint32_t samples;             // alac_yin_samples
    float threshold, rate;
};

__global__ void alac_yin_kernel(alac_yin_params p);
__global__ void alac_yin_kernel_vec(alac_yin_params p);
