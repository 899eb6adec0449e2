// alac_vad.hip -- the energy VAD of the Kaldi speaker recipes on one feature line (compute-vad-decision) and the selection of
// the voiced frames (select-voiced-frames), one launch each.  include/alacgpu.h states the mathematics, alac_vad.h the mappings
// and the order of the sum.  The threshold is float32, one IEEE operation at a time: this file is compiled with
// -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt, and the sums and products go through __fadd_rn / __fmul_rn.
// The selection moves bits.
#include "alac_vad.h"

#pragma clang fp contract(off)

namespace {

// The tree of halves over the 64 partials of a wave and over the 16 wave sums of a workgroup: alac_normalize.hip's, whose order
// the mean shares (that file's helpers are its own: the stage kernels do not include one another)
__device__ inline float wave_sum(float q) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) q = __fadd_rn(q, __shfl_xor(q, h, 64));
    return q;
}

__device__ inline float block_sum(float q, float* wsum) {
    constexpr int WAVES = ALAC_VAD_LINE_THREADS / 64;
    q = wave_sum(q);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = q;
    __syncthreads();
    float w[WAVES];
#pragma unroll
    for (int j = 0; j < WAVES; j++) w[j] = wsum[j];
#pragma unroll
    for (int h = WAVES / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int j = 0; j < h; j++) w[j] = __fadd_rn(w[j], w[j + h]);
    __syncthreads();
    return w[0];
}

__device__ inline uint64_t valid_of(const int64_t* valid, uint64_t row, uint64_t n) {
    if (!valid) return n;
    const int64_t a = valid[row];
    return a <= 0 ? 0u : ((uint64_t)a < n ? (uint64_t)a : n);
}

// A row by a team of TEAM threads, `tid` this thread's place in it: 64, a wave, or ALAC_VAD_LINE_THREADS, the workgroup
template <int TEAM>
__device__ inline void vad_row(const alac_vad_params& p, uint64_t row, uint32_t tid, float* wsum) {
    const uint64_t n = p.line_len, v = valid_of(p.valid, row, n);
    const float* E = p.energy + row * p.row_stride;
    float thr = p.threshold;
    if (p.mean_scale != 0.0f) {                                    // (the launch's: every thread takes this branch or none)
        float acc = 0.0f;
        for (uint64_t i = tid; i < v; i += TEAM) acc = __fadd_rn(acc, E[i]);
        const float sum = TEAM == 64 ? wave_sum(acc) : block_sum(acc, wsum);
        thr = __fadd_rn(p.threshold, __fmul_rn(p.mean_scale, sum / (float)v));          // (v == 0: not used)
    }
    uint8_t* mask = p.mask + row * p.mask_stride;
    const uint64_t c = p.context;
    for (uint64_t t = tid; t < n; t += TEAM) {
        uint8_t r = 0;
        if (t < v) {
            const uint64_t lo = t >= c ? t - c : 0u, hi = t + c < v ? t + c : v - 1u;
            uint32_t num = 0;
            for (uint64_t k = lo; k <= hi; k++) num += E[k] > thr ? 1u : 0u;             // (a NaN compares false)
            r = (float)num >= __fmul_rn((float)(uint32_t)(hi - lo + 1u), p.proportion) ? 1 : 0;
        }
        mask[t] = r;
    }
}

}  // namespace

// A wave per row of at most ALAC_VAD_WAVE_MAX frames (no barrier in this kernel)
__global__ __launch_bounds__(ALAC_VAD_WAVE_THREADS) void alac_vad_wave_kernel(alac_vad_params p) {
    const uint64_t row = (uint64_t)blockIdx.x * ALAC_VAD_WAVE_ROWS + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    vad_row<64>(p, row, threadIdx.x & 63u, nullptr);
}

// A workgroup per longer row
__global__ __launch_bounds__(ALAC_VAD_LINE_THREADS) void alac_vad_line_kernel(alac_vad_params p) {
    __shared__ float wsum[ALAC_VAD_LINE_THREADS / 64];
    vad_row<ALAC_VAD_LINE_THREADS>(p, blockIdx.x, threadIdx.x, wsum);
}

// The voiced frames of lines [g * per, (g + 1) * per) of row blockIdx.x / groups to the front of their lines
__global__ __launch_bounds__(ALAC_SELECT_THREADS) void alac_select_frames_kernel(alac_select_params p) {
    constexpr uint32_t WAVES = ALAC_SELECT_THREADS / 64;
    __shared__ uint32_t wcount[WAVES];
    const uint32_t row = blockIdx.x / p.groups, g = blockIdx.x % p.groups;
    const uint32_t per = p.groups == 1u ? p.lines_per_row : ALAC_SELECT_LINES;
    const uint32_t line0 = g * per, line1 = line0 + per < p.lines_per_row ? line0 + per : p.lines_per_row;
    const uint64_t n = p.line_len;
    const int64_t given = p.valid ? p.valid[row] : (int64_t)n;     // (read by every thread in front of the first barrier)
    const uint64_t v = given <= 0 ? 0u : ((uint64_t)given < n ? (uint64_t)given : n);
    const uint8_t* mask = p.mask + (uint64_t)row * p.mask_stride;
    const uint64_t first = (uint64_t)row * p.lines_per_row;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t count = 0;                                            // the voiced frames in front of the chunk
    for (uint64_t c0 = 0; c0 < n; c0 += ALAC_SELECT_CHUNK) {
        const uint64_t t = c0 + threadIdx.x;
        const bool keep = t < v && mask[t] != 0;
        const unsigned long long votes = __ballot(keep);
        if (lane == 0u) wcount[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) {
            const uint32_t k = wcount[w];
            before += w < wave ? k : 0u;
            total += k;
        }
        const uint64_t to = count + before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        for (uint32_t la = line0; la < line1; la += ALAC_SELECT_LINES) {
            float a[ALAC_SELECT_LINES];
#pragma unroll
            for (uint32_t k = 0; k < ALAC_SELECT_LINES; k++)
                if (keep && la + k < line1) a[k] = p.src[(first + la + k) * p.line_stride + t];
            __syncthreads();                                      // the chunk is read: a frame moves left, at most to its own place
#pragma unroll
            for (uint32_t k = 0; k < ALAC_SELECT_LINES; k++)
                if (keep && la + k < line1) p.out[(first + la + k) * p.line_stride + to] = a[k];
        }
        count += total;
        __syncthreads();                                          // (wcount is written again)
    }
    for (uint32_t la = line0; la < line1; la++)
        for (uint64_t i = count + threadIdx.x; i < n; i += ALAC_SELECT_THREADS) p.out[(first + la) * p.line_stride + i] = 0.0f;
    if (g == 0u && threadIdx.x == 0u) p.new_lengths[row] = given < 0 ? given : (int64_t)count;
}
