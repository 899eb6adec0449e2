// alac_cqt.h -- the constant-Q kernel (alac_cqt.hip): its launch parameters, its limits and its LDS layout, shared with the C
// ABI (alacgpu_stages.hip).  alac.net_amd/cqt.py states the mathematics and builds the table.
//
// A workgroup of four waves owns a tile of up to 32 consecutive frames of one plane (row, channel).  It loads the span of
// signal those frames cover, (tile - 1) hop + N_0 samples around their centres (N_0: the longest kernel), into LDS once --
// zeros outside the signal, nothing is reflected, each sample from global memory once per workgroup -- and every bin block
// of the tile then reads its B operand from there.
//
// The transform is D = G . frames^T on v_mfma_f32_32x32x2_f32, the instruction and the operand arrangement of the STFT tile
// body (alac_features.h): frames on the lanes.  The rows of A are the kernels of a block of ALAC_CQT_BLOCK_BINS = 16
// neighbouring bins, real and imaginary parts, 32 rows: one accumulator holds a block.  Row r of a block is the real
// ((r >> 3) & 1 == 0) or imaginary part of its bin (r >> 4) 8 + (r & 7), so that a lane finds both parts of a bin in its own
// registers (register j and j + 4) and the power needs no exchange.  B is the 32 frames of the tile.  The MFMA is a k-ordered
// chain of f32 fused multiply-adds: the bound of cqt.py rests on that, and the twin there repeats it.
//
// The ragged K: a block's loop runs over K_b taps, the even number at or above its longest kernel's length N_{16 b}, and no
// further.  The block's shorter kernels are zero-padded in the table, centred, bin k's taps at n' = c_{16 b} - c_k + n, so one
// B operand serves the block; the block's taps begin at c_0 - c_{16 b} inside a frame's span, since the frame centres
// coincide.  Zeros add nothing to a chain of finite values.  They would turn a NaN or an infinity into NaN for the whole
// block, which the specification forbids (a NaN reaches a bin through the bin's own taps only): the span load notes whether
// every sample is finite, and a tile with one that is not is evaluated by alac_cqt.hip's second path, bin by bin over each
// bin's own taps on the VALU, the same chains in the same order.
//
// The table lives in global memory and is read through L2 as fragments: block b is [K_b][32] floats, so the A operands of a
// k-step (two taps) are 64 neighbouring floats, one per lane, two full 128-byte lines.  A workgroup reads every element once,
// each by one wave; nothing of it would be shared through LDS.
//
// Balance: a workgroup takes all blocks of its tile, heaviest first across its waves (wave w: blocks w, w + 4, ...; the
// lengths fall with the block index).  A launch is as long as its slowest wave, the one with block 0: K_0 / 2 MFMAs of 64
// cycles.  All LDS is the span; there is no scratch, no atomic, every output element has one writer, all loads and stores
// are plain vector ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ALAC_CQT_THREADS = 256;
constexpr uint32_t ALAC_CQT_TILE = 32u;                 // frames of a tile: the N of v_mfma_f32_32x32x2_f32
constexpr uint32_t ALAC_CQT_BLOCK_BINS = 16u;           // bins of a block: half its M
constexpr uint32_t ALAC_CQT_MAX_BINS = 512u;
constexpr uint32_t ALAC_CQT_MAX_BLOCKS = ALAC_CQT_MAX_BINS / ALAC_CQT_BLOCK_BINS;
constexpr uint32_t ALAC_CQT_MAX_TAPS = 36864u;          // the longest kernel (cqt.py: MAX_TAPS)
constexpr uint32_t ALAC_CQT_MAX_HOP = 1u << 20;
constexpr uint32_t ALAC_CQT_LDS_FLOATS = 40832u;        // the span with its skew: the 160 KiB a CU has, less 512 bytes (the
                                                        // workgroup's vote on the span, __syncthreads_or, keeps 256 of its own)
constexpr size_t ALAC_CQT_LDS_DEFAULT = 64u << 10;      // what a launch may ask for without an attribute

// The span in LDS: sample i of it lives at i + skew * (i / hop), as in alac_features_skew: the lanes of a wave read the same
// tap of 32 neighbouring frames, hop samples apart, and with an even hop (512: every lane in one bank) one float of padding
// per hop makes the stride odd.  A tile of one frame has no neighbours and no skew.
__host__ __device__ inline uint32_t alac_cqt_skew(uint32_t hop, uint32_t tile) { return ((hop & 1u) || tile < 2u) ? 0u : 1u; }

// The floats of LDS a tile of `tile` frames takes: the span of (tile - 1) hop + n0 + 1 samples (an odd K_b is padded by one
// tap, whose sample is read: a block's taps end at c_0 - c_b + K_b <= n0 + 1 of a frame's span), and the skew
__host__ __device__ inline uint64_t alac_cqt_lds_floats(uint32_t n0, uint32_t hop, uint32_t tile) {
    const uint64_t span = (uint64_t)(tile - 1u) * hop + n0 + 1u;
    return span + (alac_cqt_skew(hop, tile) ? (span - 1u) / hop + 1u : 0u);
}

// The frames a workgroup takes: ALAC_CQT_TILE, fewer where the span of that many does not fit; one frame's always does
__host__ __device__ inline uint32_t alac_cqt_tile(uint32_t n0, uint32_t hop) {
    for (uint32_t tile = ALAC_CQT_TILE; tile > 1u; --tile)
        if (alac_cqt_lds_floats(n0, hop, tile) <= ALAC_CQT_LDS_FLOATS) return tile;
    return 1u;
}

enum { ALAC_CQT_LOG_NONE = 0, ALAC_CQT_LOG_LN = 1, ALAC_CQT_LOG_10 = 2 };

struct alac_cqt_params {
    const float* src;             // [planes, src_stride]
    uint64_t src_stride;
    uint64_t frames;              // the samples of a plane that are signal: L >= 1
    float* out;                   // [planes, n_bins, out_frames]
    uint64_t out_frames;          // 1 + frames / hop
    const float* table;           // the blocks, [K_b][32] each
    const uint32_t* lengths;      // [n_bins]: N_k (read by the second path only, and clamped there)
    uint32_t n_bins, n_blocks, hop;
    uint32_t n0, c0;              // N_0 and c_0 = N_0 / 2
    uint32_t tile;                // alac_cqt_tile(n0, hop)
    uint32_t tiles;               // ceil(out_frames / tile): blockIdx.x = plane * tiles + tile index
    uint32_t power;               // 1: sqrt(P), 2: P
    uint32_t log_mode;
    float floor;
    uint32_t blk_k[ALAC_CQT_MAX_BLOCKS];       // K_b: even
    uint32_t blk_off[ALAC_CQT_MAX_BLOCKS];     // where block b begins in the table, in floats
    uint32_t blk_start[ALAC_CQT_MAX_BLOCKS];   // c_0 - c_{16 b}: where its taps begin in a frame's span
};

__global__ void alac_cqt_kernel(alac_cqt_params p);
