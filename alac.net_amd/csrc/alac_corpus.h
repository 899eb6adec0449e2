// alac_corpus.h -- the crop planner's launch parameters (alac_corpus.hip), shared with the C ABI (alacgpu_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t ALAC_PLAN_PAD_CFG = 0xFFFFu;   // a padding entry's cfg_idx: no row of any ctx (parse_meta: badcfg)
constexpr uint32_t ALAC_PLAN_MAX_SKIP = 16384u;   // src_skip is clamped to the longest frame (frames behind it are zeros)
constexpr int ALAC_PLAN_THREADS = 256;            // one wave per crop, four crops per workgroup

struct alac_plan_params {
    // the resident tables of a corpus (include/alacgpu.h: alacgpu_plan_crops_device)
    const uint64_t* pkt_offset;   // [P] byte offset of a packet into the resident blob
    const uint32_t* pkt_size;     // [P]
    const uint64_t* pkt_end;      // [P] inclusive prefix sum of the durations within the packet's file
    const uint32_t* file_first;   // [F + 1] first global packet of a file
    const uint16_t* file_cfg;     // [F]
    uint32_t n_files;
    // the crops of this call
    const uint32_t* crop_file;    // [B]
    const uint64_t* crop_offset;  // [B]
    uint32_t n_crops;
    uint32_t crop_frames;         // L
    uint32_t entries_per_crop;    // K
    uint64_t dst_stride;
    // the plan: B * K entries, crop-major
    uint64_t* offsets;
    uint32_t* sizes;
    uint16_t* cfg_idx;
    uint64_t* dst_first;
    uint32_t* dst_frames;
    uint32_t* src_skip;
    int64_t* lengths;             // [B]
};

__global__ void alac_plan_crops_kernel(alac_plan_params p);
