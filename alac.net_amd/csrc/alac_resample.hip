// alac_resample.hip -- the polyphase resampler behind the decode (alacgpu_resample_device): a Hann-windowed sinc, a : b the
// reduced ratio of the two rates, as a table of b phases of N = 2 * width + 1 weights (alac.net_amd/resample.py states the
// filter).  Output frame j = i + b m reads the N source frames from m a + d0[i] on; that first frame, floor(j a / b) - width,
// grows with j, so a run of output frames reads one run of source frames.
//
// A workgroup owns tiles of `tile` consecutive output frames of one (row, output channel).  It keeps the whole weight table in
// LDS (at most 64 KiB, loaded once per workgroup and used for up to eight tiles) and, per tile, the source span the tile
// reads: neighbouring lanes load neighbouring frames, each frame once, and the bounds test -- a frame outside [origin,
// origin + valid) is zero whatever the memory holds -- and the mono sum happen on that load.  A thread then produces an
// output frame with N fused multiply-adds in ascending tap order out of LDS: phase rows are N floats apart, N odd, so the
// lanes of a wave read the table without bank conflicts, and their source runs start a / b frames apart.  Neighbouring lanes
// store neighbouring output frames.  Every output element has exactly one writer; there are no atomics, and all loads and
// stores are plain vector ones.  The arithmetic is nothing (N flops per output frame): what the shape is for is one pass over
// the source and full cache lines both ways.
#include "alac_resample.h"

__global__ __launch_bounds__(ALAC_RESAMPLE_THREADS) void alac_resample_kernel(alac_resample_params p) {
    extern __shared__ __align__(16) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t N = 2u * p.width + 1u;
    const uint32_t table = p.b * N;
    float* const w = lds;
    float* const xs = lds + ((table + 3u) & ~3u);

    // blockIdx.x: (row, output channel, group of tiles), the group fastest
    const uint32_t out_channels = p.mono ? 1u : p.channels;
    const uint32_t tiles = (uint32_t)((p.out_frames + p.tile - 1u) / p.tile);
    const uint32_t groups = (tiles + p.tiles_per_wg - 1u) / p.tiles_per_wg;
    const uint32_t group = blockIdx.x % groups;
    const uint32_t plane = blockIdx.x / groups;
    const uint32_t c = plane % out_channels;
    const uint64_t row = plane / out_channels;

    for (uint32_t i = tid; i < table; i += ALAC_RESAMPLE_THREADS) w[i] = p.weights[i];

    const int64_t origin = p.src_origin[row];
    int64_t valid = p.src_valid[row];
    valid = valid < 0 ? 0 : (valid > (int64_t)p.src_stride ? (int64_t)p.src_stride : valid);
    const int64_t first = p.out_first[row];
    // the resampled signal has ceil(b (origin + valid) / a) frames: j is one of them iff 0 <= j and j a < b (origin + valid)
    const int64_t end_b = (origin + valid) * (int64_t)p.b;
    const bool two = p.mono && p.channels == 2u;
    const float* const s0 = p.src + (row * p.channels + c) * p.src_stride;
    const float* const s1 = s0 + p.src_stride;
    float* const dst = p.out + (row * out_channels + c) * p.out_frames;

    for (uint32_t t = 0; t < p.tiles_per_wg; ++t) {
        const uint64_t k0 = ((uint64_t)group * p.tiles_per_wg + t) * p.tile;
        if (k0 >= p.out_frames) break;
        // the tile's first frame j0 = i0 + b m0 (floored: a j below 0 is written as zero, but its taps must not wrap)
        const int64_t j0 = first + (int64_t)k0;
        int64_t m0 = j0 / (int64_t)p.b;
        int32_t i0 = (int32_t)(j0 - m0 * (int64_t)p.b);
        if (i0 < 0) {
            i0 += (int32_t)p.b;
            m0 -= 1;
        }
        const int32_t d00 = p.d0[i0];
        const int64_t s_lo = m0 * (int64_t)p.a + d00;      // the first source frame of the tile
        __syncthreads();                                    // (the tile before has been computed)
        for (uint32_t idx = tid; idx < p.span; idx += ALAC_RESAMPLE_THREADS) {
            const int64_t rel = s_lo + idx - origin;
            float v = 0.0f;
            if (rel >= 0 && rel < valid) {
                v = s0[rel];
                if (two) v = (v + s1[rel]) * 0.5f;
            }
            xs[idx] = v;
        }
        __syncthreads();
        const uint64_t left = p.out_frames - k0;
        const uint32_t n_out = left < p.tile ? (uint32_t)left : p.tile;
        for (uint32_t k = tid; k < n_out; k += ALAC_RESAMPLE_THREADS) {
            const uint32_t ii = (uint32_t)i0 + k;
            const uint32_t mo = ii / p.b;
            const uint32_t i = ii - mo * p.b;
            uint32_t rel = mo * p.a + (uint32_t)(p.d0[i] - d00);
            rel = rel > p.span - N ? p.span - N : rel;      // (a table that is what resample.py makes it never gets here)
            const float* const wr = w + i * N;
            const float* const x = xs + rel;
            float acc = 0.0f;
            for (uint32_t n = 0; n < N; ++n) acc = __builtin_fmaf(wr[n], x[n], acc);
            const int64_t j = j0 + (int64_t)k;
            dst[k0 + k] = (j >= 0 && j * (int64_t)p.a < end_b) ? acc : 0.0f;
        }
    }
}
