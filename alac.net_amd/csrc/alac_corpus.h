// alac_corpus.h -- the launch parameters of the crop planner, of the packet compaction and of the packet staging
// (alac_corpus.hip), shared with the C ABI (alacgpu_api.hip).
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
    const uint32_t* crop_frames_each;   // [B] alac_plan_crops_frames_kernel only: a length per crop, L their bound
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
__global__ void alac_plan_crops_frames_kernel(alac_plan_params p);

// ---- packet compaction (include/alacgpu.h: alacgpu_compact_packets_device) ----------------------------------------------------
constexpr int ALAC_SCAN_THREADS = 256;
constexpr uint32_t ALAC_SCAN_ITEMS = 8;                                      // consecutive elements per thread
constexpr uint32_t ALAC_SCAN_TILE = ALAC_SCAN_THREADS * ALAC_SCAN_ITEMS;     // elements per workgroup: 2048
constexpr int ALAC_COPY_THREADS = 256;
constexpr uint32_t ALAC_COPY_CHUNKS = 4;                                     // 16-byte destination chunks per thread and tile
constexpr uint64_t ALAC_COPY_TILE = (uint64_t)ALAC_COPY_THREADS * ALAC_COPY_CHUNKS * 16u;   // destination bytes per tile: 16 KiB

// One level of the scan.  T = uint32_t: the packet sizes (one above `slot_bytes` counts as 0; the _stage kernels count a size
// rounded up to 16 when the packet at src_offset[i] lies wholly inside one of the two source parts, else 0); T = uint64_t: the
// sums of the level below.  alac_scan_sums_kernel writes a tile's sum to sums[tile]; alac_scan_tiles_kernel writes out[i] =
// add + tile_base[tile] (0 if null) + the sum of the tile's elements in front of i, and the workgroup of the last tile the
// grand total to total[0] if that is not null (only asked of a single-tile launch).  in == out is allowed.
template <class T>
struct alac_scan_params {
    const T* in;
    uint64_t n;
    uint64_t slot_bytes;
    const uint64_t* src_offset;   // the _stage kernels only: [n] a packet's offset into the source space, and the two parts'
    uint64_t lo_bytes, hi_bytes;  // sizes
    uint64_t* sums;
    const uint64_t* tile_base;
    uint64_t add;
    uint64_t* out;
    uint64_t* total;
};

struct alac_copy_params {
    const uint8_t* packets;       // packet p at packets + p * slot_bytes, 16-byte aligned
    uint64_t slot_bytes;          // a multiple of 16
    const uint32_t* sizes;        // [n]
    const uint64_t* pkt_offset;   // [n] as the scan left it: base + the counted sizes in front
    const uint64_t* total;        // [1]
    uint32_t n_packets;
    uint8_t* blob;
    uint64_t base;
    uint64_t capacity;
};

__global__ void alac_scan_sums_u32_kernel(alac_scan_params<uint32_t> p);
__global__ void alac_scan_sums_u64_kernel(alac_scan_params<uint64_t> p);
__global__ void alac_scan_tiles_u32_kernel(alac_scan_params<uint32_t> p);
__global__ void alac_scan_tiles_u64_kernel(alac_scan_params<uint64_t> p);
__global__ void alac_compact_copy_kernel(alac_copy_params p);

// ---- packet staging (include/alacgpu.h: alacgpu_stage_packets_device) ---------------------------------------------------------
constexpr int ALAC_STAGE_THREADS = 256;
constexpr uint32_t ALAC_STAGE_CHUNKS = 8;   // 16-byte destination chunks per thread and tile (the only count measured: DESIGN.md section 3)
constexpr uint64_t ALAC_STAGE_TILE = (uint64_t)ALAC_STAGE_THREADS * ALAC_STAGE_CHUNKS * 16u;   // destination bytes per tile

struct alac_stage_params {
    const uint8_t* lo;            // offset x < lo_bytes of the source space is lo[x] (device memory), 16-byte aligned
    const uint8_t* hi;            // ... every other one hi[x - lo_bytes] (the device view of page-locked memory, or device memory)
    uint64_t lo_bytes, hi_bytes;
    const uint64_t* src_offset;   // [n]
    const uint32_t* sizes;        // [n]
    const uint64_t* stage_offset; // [n] as the scan left it: the counted, rounded sizes in front
    const uint64_t* total;        // [1]
    uint32_t n_packets;
    uint8_t* stage;               // 16-byte aligned
    uint64_t capacity;
};

__global__ void alac_scan_sums_stage_kernel(alac_scan_params<uint32_t> p);
__global__ void alac_scan_tiles_stage_kernel(alac_scan_params<uint32_t> p);
__global__ void alac_stage_copy_kernel(alac_stage_params p);
