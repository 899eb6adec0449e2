// alac_reverb.h -- the launch parameters, the block length, the layout of the spectra and the order of the sums of the room
// reverberation between the crops and the noise mix (alac_reverb.hip), shared with the C ABI (alacgpu_stages.hip).  The data
// is float32, planar: the signal and the result [rows, channels, stride], the impulse responses [rows, rir_channels,
// rir_stride] with rir_channels 1 or channels; the first `frames` (`rir_frames`) elements of a plane are data.
// include/alacgpu.h states the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A uniformly partitioned overlap-save convolution.  A block is ALAC_REVERB_N frames, transformed as ALAC_REVERB_N complex
// points (the imaginary parts of the input are 0) by a radix-4 transform in LDS: 32 KiB a workgroup of ALAC_REVERB_THREADS.
// The hop is ALAC_REVERB_HOP = N / 2.  With H the hop:
//   block j of a signal plane holds x[(j - 1) H + t], t < N, 0 outside 0 .. v;     j = 0 .. ceil(v / H)
//   partition p of an impulse response plane holds h[p H + t], t < H and p H + t < vh, 0 elsewhere;   p < ceil(vh / H)
//   block m of the convolution w[n] = sum over k of h[k] x[n - k], n = m H + s, is elements H + s, s < H, of the inverse
//   transform of sum over p of X[m - p] . H[p] (ascending p, those p for which both spectra exist), divided by N.
// The forward transform is decimation in frequency: six stages of span L = N / 4, N / 16 .. 1.  Butterfly q < N / 4 of a stage
// takes the elements i0 = (q / L) 4 L + q mod L, i0 + L, i0 + 2 L, i0 + 3 L = a, b, c, d and writes
//   i0: (a + c) + (b + d)         i0 + L:  ((a - c) - i (b - d)) w^j
//   i0 + 2 L: ((a + c) - (b + d)) w^2j     i0 + 3 L: ((a - c) + i (b - d)) w^3j        j = q mod L, w = exp(-2 pi i / (4 L))
// so a spectrum is in base-4 digit-reversed order, in which it is stored, multiplied and fed to the inverse transform: the
// stages in the opposite order, each the conjugate transpose of its forward stage (the conjugate twiddles first, then the
// butterfly with i for -i).  The twiddles are table[k] = exp(-2 pi i k / N), k < N, computed in float64 and rounded once
// (alac.net_amd/reverb.py: twiddles()); w^(r j) of the stage of span L is table[r j N / (4 L)].  A complex product is
// (ar br - ai bi, ar bi + ai br), every operation rounded once, none fused.
//
// The spectra scratch, in float2: for row r the ALAC_REVERB_N-point spectra of its channels * x_blocks signal blocks (channel c,
// block j at c * x_blocks + j), then of its rir_channels * rir_parts partitions; behind all rows' spectra one alac_reverb_row
// per row.  x_blocks = ceil(frames / H) + 1 and rir_parts = ceil(rir_frames / H) are those of the call's shape; a block
// without a frame below v and a partition without one below vh are neither written nor read.
//
// The verdict of a row, by workgroup `units - 1` of its share of the analyse launch: with vh the valid frames of the impulse
// response, thread t of ALAC_REVERB_THREADS takes the frames k = t, t + THREADS, ... < vh of channel 0, then of channel 1:
//   q[t] = ((0 + h[0, t]^2) + h[0, t + THREADS]^2) + ... the squares rounded once; best[t] the first k of channel 0 whose
//   |h[0, k]| is largest.
// The ALAC_REVERB_THREADS partials are added as a tree of halves, q[t] += q[t + s] for s = THREADS / 2 .. 1, and the maxima
// joined by the same tree (the larger value, of equal values the smaller index).  e = q[0] / rir_channels, g = 1 / sqrt(e),
// division and root correctly rounded; the row is left alone where v == 0, vh == 0, e == 0 or e is not finite.
constexpr int ALAC_REVERB_THREADS = 256;
constexpr uint32_t ALAC_REVERB_N = 4096u;
constexpr uint32_t ALAC_REVERB_STAGES = 6u;
constexpr uint32_t ALAC_REVERB_HOP = ALAC_REVERB_N / 2u;
static_assert(1u << (2u * ALAC_REVERB_STAGES) == ALAC_REVERB_N, "the transform is radix 4: N is a power of 4");
static_assert(ALAC_REVERB_N / 4u % ALAC_REVERB_THREADS == 0u && ALAC_REVERB_N / 2u >= (uint32_t)ALAC_REVERB_THREADS,
              "a thread takes whole butterflies of every stage and pairs of bins of a spectrum");

struct alac_reverb_row {
    float g;                      // 1 / sqrt(e)
    uint32_t live;                // 0: the row is left alone
    uint64_t d;                   // the direct path
};

__host__ __device__ inline uint64_t alac_reverb_x_blocks(uint64_t frames) { return (frames + ALAC_REVERB_HOP - 1u) / ALAC_REVERB_HOP + 1u; }
__host__ __device__ inline uint64_t alac_reverb_parts(uint64_t rir_frames) { return (rir_frames + ALAC_REVERB_HOP - 1u) / ALAC_REVERB_HOP; }
// the blocks of the convolution a synthesise launch covers: those of n < frames + rir_frames - 1
__host__ __device__ inline uint64_t alac_reverb_out_blocks(uint64_t frames, uint64_t rir_frames) {
    return (frames + rir_frames - 1u + ALAC_REVERB_HOP - 1u) / ALAC_REVERB_HOP;
}

struct alac_reverb_params {
    const float* src;             // [rows, channels, stride]
    float* out;                   // the same layout; may be src
    const float* rir;             // [rows, rir_channels, rir_stride]
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), frames), null: frames
    const int64_t* rir_valid;     // [rows] or null: vh likewise, of rir_frames
    const float2* twiddles;       // [ALAC_REVERB_N]
    float2* spectra;              // [rows, units - 1, ALAC_REVERB_N]
    alac_reverb_row* verdict;     // [rows]
    uint32_t channels, rir_channels;
    uint64_t stride, rir_stride, frames, rir_frames;
    uint32_t x_blocks, rir_parts; // alac_reverb_x_blocks(frames), alac_reverb_parts(rir_frames)
    uint32_t units;               // channels * x_blocks + rir_channels * rir_parts + 1: analyse, blockIdx.x = row * units + unit
    uint32_t out_blocks;          // alac_reverb_out_blocks: synthesise, blockIdx.x = (row * channels + c) * out_blocks + m
};

__global__ void alac_reverb_analyse_kernel(alac_reverb_params p);
__global__ void alac_reverb_synth_kernel(alac_reverb_params p);
