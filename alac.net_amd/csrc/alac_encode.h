// alac_encode.h -- the GPU encoder's launch parameters (alac_encode.hip), shared with the C ABI (alacgpu_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alac_kernels.h"

// Items of one packet in the workspace (see alac_encode.hip): 21 header fields, then per frame one item of low bytes (or
// of raw samples in an escape packet), one of channel A's Rice symbols, one of channel B's, then the END tag.
constexpr uint32_t ALAC_ENC_HDR_ITEMS = 21;
constexpr int ALAC_ENC_THREADS = 64;     // one wave per packet
__host__ __device__ inline uint64_t alac_enc_items(uint32_t smax) { return ALAC_ENC_HDR_ITEMS + 3ull * smax + 1ull; }

struct alac_encode_params {
    const void* pcm;              // int32 or float32 source tensor
    uint64_t src_elems;
    uint64_t plane_stride;        // planar: channel c of frame t at c * plane_stride + t
    uint32_t channels;            // 1 or 2 (every cfg of the ctx has this many)
    uint32_t layout;              // ALACGPU_DST_INTERLEAVED / ALACGPU_DST_PLANAR
    uint32_t dtype;               // ALACGPU_DST_INT32 / ALACGPU_DST_FLOAT32
    uint32_t n_packets;
    uint32_t first_packet;        // this launch: packets first_packet + blockIdx.x (one workspace slot per workgroup)
    const uint64_t* src_first;    // frame index of packet p's first frame
    const uint32_t* src_frames;   // frames in packet p
    const uint16_t* cfg_idx;
    const alacgpu_cfg_dev* cfgs;
    uint32_t n_cfgs;
    uint32_t smax;                // the largest max_samples_per_frame of the cfgs (<= 16384): sizes the workspace
    uint8_t* packets;             // packet p at packets + p * slot_bytes (16-byte aligned, slot_bytes a multiple of 16)
    uint64_t slot_bytes;
    uint32_t* sizes;
    int32_t* status;
    uint64_t* ws_code;            // per workgroup: alac_enc_items(smax) codes ...
    uint32_t* ws_pos;             // ... and alac_enc_items(smax) + 1 bit positions
};

// One round of up to gridDim.x packets is the three launches in this order on one stream (alacgpu_api.hip).
__global__ void alac_encode_analyse_kernel(alac_encode_params p);
__global__ void alac_encode_codes_kernel(alac_encode_params p);
__global__ void alac_encode_emit_kernel(alac_encode_params p);
