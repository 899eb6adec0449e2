// alac_rir.h -- the launch parameters, the constants and the order of the image-source kernel (alac_rir.hip), shared with the C
// ABI (alacgpu_stages.hip).  geometry is float64 [rows, 9] (room, source, microphone in metres), beta float32 [rows, 6], the
// output float32 [rows, out_stride] of which the first `frames` of a row are written, lengths int32 [rows].
// alac.net_amd/rir.py states every operation in order; its float32 twin follows them and equals the kernel bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A workgroup is one wave: it owns a row and ALAC_RIR_TILE consecutive taps, a lane a tap.  It decides the row's refusal
// itself (every workgroup of a row alike; the first writes the length), then walks the candidate box in ascending (nx, ny):
// for 64 values of ny at a time the lanes solve, from one square root each, the nz that can lie in the tile's shell of
// distances (the union over the eight p, widened by one; the hole inside the shell likewise narrowed), then the wave takes
// the pairs one after the other and 64 candidates (nz, p) at a time: a lane evaluates its candidate's distance, delay and
// k0 in float64 and tests exactly whether it is of the order asked for and reaches the tile; a ballot compacts those that
// do, in order, into a list in LDS.  At 64 or more the list is flushed: a lane computes an image's amplitude and its three
// polynomials, then every lane adds, image after image, those that reach its tap.  No image list leaves the workgroup, no
// atomics; a tap's sum is in ascending (nx, ny, nz, p) whatever the tiling.
constexpr int ALAC_RIR_THREADS = 64;
constexpr uint32_t ALAC_RIR_TILE = 64u;
constexpr uint32_t ALAC_RIR_MAX_TAPS = 127u;                 // odd, 3 ..; the window's table is (taps div 2) + 1 <= 64 entries
constexpr uint32_t ALAC_RIR_MAX_FRAMES = 1u << 20;
constexpr double ALAC_RIR_LIMIT = 33554432.0;                // 2^25 candidates of a row's box; more: the row is refused (rir.LIMIT)
constexpr double ALAC_RIR_MAX_QUOTIENT = 1048576.0;          // dmax / (2 L_a) at or above it: refused at once
constexpr uint32_t ALAC_RIR_LIST = 128u;                     // the list in LDS: flushed at 64, at most 63 + 64 entries

struct alac_rir_params {
    const double* geometry;       // [rows, 9]
    const float* beta;            // [rows, 6]
    float* out;                   // [rows, out_stride]
    int32_t* lengths;             // [rows]: frames, or 0 where the row is refused
    uint64_t out_stride;
    uint32_t frames, taps, tiles; // tiles a row: ceil(frames / ALAC_RIR_TILE)
    int32_t max_order;            // -1: every order
    double scale;                 // sample_rate / sound_speed, samples a metre
    float tw;                     // float(2 pi / taps)
    float cw[64], sw[64];         // float (cos, sin)(2 pi j / taps), j <= taps div 2, computed in double
};

__global__ void alac_rir_shoebox_kernel(alac_rir_params p);
