// alac_stretch.h -- the launch parameters, the transform, the layout of the spectra and the order of the sums of the phase
// vocoder behind the crops (alac_stretch.hip), shared with the C ABI (alacgpu_stages.hip).  The data is float32, planar: the
// signal [rows, channels, src_stride], the result [rows, channels, out_stride].  include/alacgpu.h states the arithmetic,
// alac.net_amd/pitch.py restates it operation by operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// N = n_fft is 512, 1024 or 2048, the hop H = N / 4, K = N / 2 + 1 bins.  A row of v valid frames at the factor p / q has
// T = 1 + v / H STFT frames, T' = ceil(T p / q) output frames and Ls = (2 v p + q) / (2 q) output samples; it is live where
// p != q, both are in 1 .. 2^20 and v > N / 2.  Three launches:
//   analyse     one workgroup per (plane, frame t < 1 + frames / H): z[n] = (window[n] * x[refl(t H - N / 2 + n)], 0), the
//               N-point complex transform in LDS, the bins 0 .. N / 2 stored in natural order to X [planes, t_max, K].
//               The workgroup of frame 0 of channel 0 writes the row's new length.
//   scan        one lane per (plane, bin): j = 0 .. min(T', t_cap) - 1 in ascending order, Y [planes, t_cap, K].
//   synthesise  one workgroup per (plane, tile of ALAC_STRETCH_TILE_HOPS hops of output): the frames j = first hop - 1 ..
//               last hop + 2 that exist, in ascending order: the spectrum made Hermitian, the inverse transform,
//               acc[n] += window[i] * (re z[i] / N) in LDS; then y[n] = acc[n] / env[n], env the sum of window[i]^2 over the
//               same frames in the same order; 0 from min(Ls, (T' - 1) H + 1) up to out_frames.
// The transform: for N = 512 and 2048 a radix-2 decimation-in-frequency stage (q < N / 2: a = z[q], b = z[q + N / 2];
// z[q] = a + b, z[q + N / 2] = (a - b) table[q]) and then alac_reverb.h's radix-4 stages of span L = N / 8 .. 1 over both
// halves; for 1024 the radix-4 stages from L = N / 4.  Bin k ends at alac_stretch_pos<N>(k): the base-4 digits of k (of k / 2,
// in the half k % 2 names) reversed.  The inverse is the stages' conjugate transposes in the opposite order.  The tables, made
// by the host in float64 and rounded once: table[k] = exp(-2 pi i k / N), window[n] = 0.5 - 0.5 cos(2 pi n / N).
constexpr uint32_t ALAC_STRETCH_TILE_HOPS = 4u;
constexpr uint32_t ALAC_STRETCH_SCAN_THREADS = 256u;
constexpr uint32_t ALAC_STRETCH_COPY_THREADS = 256u;
constexpr uint32_t ALAC_STRETCH_COPY_TILE = 4096u;
constexpr uint32_t ALAC_STRETCH_MAX_TERM = 1u << 20;      // p and q of a live row

__host__ __device__ constexpr uint32_t alac_stretch_threads(uint32_t n_fft) { return n_fft / 4u < 256u ? n_fft / 4u : 256u; }
__host__ __device__ inline uint64_t alac_stretch_frames(uint64_t v, uint32_t n_fft) { return 1u + v / (n_fft / 4u); }
// the frames of Y a plane holds: no sample below out_frames reads a frame at or behind it
__host__ __device__ inline uint64_t alac_stretch_cap(uint64_t out_frames, uint32_t n_fft) { return out_frames / (n_fft / 4u) + 4u; }
__host__ __device__ inline uint64_t alac_stretch_tiles(uint64_t out_frames, uint32_t n_fft) {
    const uint64_t tile = (uint64_t)ALAC_STRETCH_TILE_HOPS * (n_fft / 4u);
    return (out_frames + tile - 1u) / tile;
}

struct alac_stretch_params {
    const float* src;             // [rows, channels, src_stride]
    float* out;                   // [rows, channels, out_stride]
    const int32_t* p;             // [rows]
    const int32_t* q;             // [rows]
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), frames), null: frames
    int64_t* valid_out;           // [rows]: min(Ls, out_frames) of a live row, min(valid[r], frames) of any other
    const float2* table;          // [n_fft]
    const float* window;          // [n_fft]
    float2* X;                    // [rows * channels, t_max, K]
    float2* Y;                    // [rows * channels, t_cap, K]
    uint64_t src_stride, out_stride, frames, out_frames;
    uint64_t chains;              // rows * channels * K: the scan's lanes
    uint32_t channels;
    uint32_t t_max;               // alac_stretch_frames(frames, n_fft)
    uint32_t t_cap;               // alac_stretch_cap(out_frames, n_fft)
    uint32_t out_tiles;           // alac_stretch_tiles(out_frames, n_fft)
};

template <uint32_t N> __global__ void alac_stretch_analyse_kernel(alac_stretch_params p);
template <uint32_t N> __global__ void alac_stretch_scan_kernel(alac_stretch_params p);
template <uint32_t N> __global__ void alac_stretch_synth_kernel(alac_stretch_params p);
// the three kernels of n_fft (512, 1024 or 2048), for the host
void alac_stretch_kernels(uint32_t n_fft, const void*& analyse, const void*& scan, const void*& synth);

// out[r, c, n] = src[r, c, n] for n < min(max(valid[r], 0), frames): the rows of one planar array into another
struct alac_copy_rows_params {
    const float* src;             // [rows, channels, src_stride]
    float* out;                   // [rows, channels, out_stride]
    const int64_t* valid;         // [rows]
    uint64_t src_stride, out_stride, frames;
    uint32_t channels, tiles;     // tiles of ALAC_STRETCH_COPY_TILE frames a plane
};

__global__ void alac_copy_rows_kernel(alac_copy_rows_params p);
