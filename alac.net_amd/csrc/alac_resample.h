// alac_resample.h -- the launch parameters of the polyphase resampler (alac_resample.hip), shared with the C ABI
// (alacgpu_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ALAC_RESAMPLE_THREADS = 256;
constexpr uint32_t ALAC_RESAMPLE_MAX_TABLE = 16384u;    // weights of a table: 64 KiB of LDS
constexpr uint32_t ALAC_RESAMPLE_MAX_TILE = 1024u;      // output frames of a tile: four per thread
constexpr uint32_t ALAC_RESAMPLE_MAX_TILES_PER_WG = 8u; // consecutive tiles a workgroup takes with one load of the table
constexpr size_t ALAC_RESAMPLE_LDS_PREFERRED = 64u << 10;   // two workgroups and more per CU
constexpr size_t ALAC_RESAMPLE_LDS_MAX = 160u << 10;        // what a CU has

// The source frames a tile of `tile` output frames reads: floor(j a / b) - width .. floor((j + tile - 1) a / b) + width.
__host__ __device__ inline uint64_t alac_resample_span(uint64_t tile, uint64_t a, uint64_t b, uint64_t width) {
    return ((tile - 1u) * a) / b + 2u * width + 2u;
}

// What every resample launch has: the rows' source and output and the placement of the workgroups.  The three parameter structs
// contain it; the host fills it once (alacgpu_stages.hip: resample<P>).
struct alac_resample_io {
    const float* src;             // [rows, channels, src_stride]
    uint64_t src_stride;
    const int64_t* src_origin;    // [rows] the absolute source frame of element 0
    const int64_t* src_valid;     // [rows] the frames behind it that hold signal
    const int64_t* out_first;     // [rows] the absolute target frame of output element 0
    float* out;                   // [rows, mono ? 1 : channels, out_frames]
    uint64_t out_frames;
    uint32_t channels;
    uint32_t mono;
    uint32_t tile;                // output frames per tile, the same for every row, at most ALAC_RESAMPLE_MAX_TILE
    uint32_t tiles_per_wg;
};

struct alac_resample_params {
    alac_resample_io io;
    uint32_t a, b, width;         // (the scalars behind io's: a workgroup reads them with the same load)
    uint32_t span;                // alac_resample_span(tile, a, b, width)
    const int32_t* d0;            // [b]
    const float* weights;         // [b, 2 * width + 1]
};

__global__ void alac_resample_kernel(alac_resample_params p);

// ---- a table per row (include/alacgpu.h: alacgpu_resample_rows_device) ---------------------------------------------------------
// One table of such a call: alacgpu_resample_table of include/alacgpu.h, field for field
struct alac_resample_table {
    uint32_t a, b, width;
    uint32_t d0_first;            // its d0[b] starts at this element of the call's d0 array
    uint32_t weights_first;       // its weights[b, 2 * width + 1] at this element of the call's weights array
};

struct alac_resample_rows_params {
    alac_resample_io io;
    const alac_resample_table* tables;   // [n_tables]
    const int32_t* d0;            // the tables' d0 arrays, one behind the other
    const float* weights;         // ... and their weights
    const uint32_t* row_table;    // [rows] the table of a row; n_tables and above: the row is written as zeros
    uint32_t n_tables;
    uint32_t lds_floats;          // the dynamic LDS of the launch: the largest table (rounded up to 4) + span of a tile
};

__global__ void alac_resample_rows_kernel(alac_resample_rows_params p);

// ---- a ratio per row, no table (include/alacgpu.h: alacgpu_resample_ratio_rows_device) -----------------------------------------
// One ratio of such a call: alacgpu_resample_ratio of include/alacgpu.h, field for field
struct alac_resample_ratio {
    uint32_t a, b, width;         // a == 0: the rows that name it are skipped
};

constexpr uint32_t ALAC_RESAMPLE_RATIO_MAX_WIDTH = (uint32_t)(ALAC_RESAMPLE_LDS_MAX / sizeof(float) - 2u) / 2u;   // a frame's span fits

struct alac_resample_ratio_params {
    alac_resample_io io;
    const alac_resample_ratio* ratios;   // [n_ratios]
    const uint32_t* row_ratio;    // [rows] the ratio of a row; n_ratios and above: the row is skipped
    uint32_t n_ratios;
    uint32_t lds_floats;          // the dynamic LDS of the launch: the largest span of a tile over the call's ratios
};

__global__ void alac_resample_ratio_rows_kernel(alac_resample_ratio_params p);
