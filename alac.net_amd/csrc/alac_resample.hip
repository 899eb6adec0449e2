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
//
// alacgpu_resample_rows_device is the same workgroup with a table per row: a row names one of the call's tables, the
// workgroup reads that table's descriptor (it is workgroup-uniform: scalar loads), loads that table into LDS and uses that
// table's span; the tile is the call's.  Row for row the arithmetic is the one above, so a row is bit for bit what the
// one-table call gives for it.  A row that names no table is written as zeros.
//
// alacgpu_resample_ratio_rows_device (the end of this file) has no table at all: a ratio per row, and every tap's weight
// evaluated where it is used.  The three kernels share the placement of the workgroups, the row view and one tile body
// (resample_tiles), to which each passes where a tile starts and what a frame's taps weigh.
#include <type_traits>

#include "alac_resample.h"

namespace {

// The table a workgroup works with and the source span a tile of it reads
struct resample_table_view {
    const int32_t* d0;            // [b]
    const float* weights;         // [b, 2 * width + 1]
    uint32_t a, b, width;
    uint32_t span;                // alac_resample_span(tile, a, b, width)
};

// blockIdx.x: (row, output channel, group of tiles), the group fastest
__device__ __forceinline__ void resample_place(const alac_resample_io& p, uint32_t& group, uint32_t& c, uint64_t& row) {
    const uint32_t out_channels = p.mono ? 1u : p.channels;
    const uint32_t tiles = (uint32_t)((p.out_frames + p.tile - 1u) / p.tile);
    const uint32_t groups = (tiles + p.tiles_per_wg - 1u) / p.tiles_per_wg;
    group = blockIdx.x % groups;
    const uint32_t plane = blockIdx.x / groups;
    c = plane % out_channels;
    row = plane / out_channels;
}

// One (row, output channel c) of a launch, for a ratio whose target side is b
struct resample_row {
    int64_t origin, valid;        // the source frames [origin, origin + valid) hold signal, valid clamped into 0 .. src_stride
    int64_t first;                // the absolute target frame of output element 0
    int64_t end_b;                // the resampled signal has ceil(b (origin + valid) / a) frames: j is one iff 0 <= j and j a < end_b
    bool two;                     // two channels become their mean on the load
    const float *s0, *s1;
    float* dst;
};

__device__ __forceinline__ resample_row resample_row_of(const alac_resample_io& p, uint32_t c, uint64_t row, uint32_t b) {
    resample_row r;
    r.origin = p.src_origin[row];
    const int64_t valid = p.src_valid[row];
    r.valid = valid < 0 ? 0 : (valid > (int64_t)p.src_stride ? (int64_t)p.src_stride : valid);
    r.first = p.out_first[row];
    r.end_b = (r.origin + r.valid) * (int64_t)b;
    r.two = p.mono && p.channels == 2u;
    r.s0 = p.src + (row * p.channels + c) * p.src_stride;
    r.s1 = r.s0 + p.src_stride;
    r.dst = p.out + (row * (p.mono ? 1u : p.channels) + c) * p.out_frames;
    return r;
}

// The source span of a tile into LDS: xs[idx] = x[s_lo + idx], idx < span -- a frame outside [origin, origin + valid) is zero
// whatever the memory holds, two channels become their mean here -- between the barriers that fence it from the tile before.
__device__ __forceinline__ void resample_stage(float* xs, uint32_t span, int64_t s_lo, const resample_row& r) {
    __syncthreads();                                        // (the tile before has been computed)
    for (uint32_t idx = threadIdx.x; idx < span; idx += ALAC_RESAMPLE_THREADS) {
        const int64_t rel = s_lo + idx - r.origin;
        float v = 0.0f;
        if (rel >= 0 && rel < r.valid) {
            v = r.s0[rel];
            if (r.two) v = (v + r.s1[rel]) * 0.5f;
        }
        xs[idx] = v;
    }
    __syncthreads();
}

// The workgroup's tiles of (row, output channel c) with the ratio a : b, N taps a frame and `span` source frames a tile in xs.
// The tile's first frame j0 gives num j0 = q0 b + r0, floored (a j below 0 is written as zero, but its taps must not wrap); the
// kernels say the rest: start(q0, r0) is the first source frame of the tile, and frame(r0, k, rel) sets rel, where in the span
// the taps of frame j0 + k start, and returns its weights: weight(n) is tap n's, asked for once each in ascending n.  Every
// thread calls start once per tile, in front of that tile's frame calls: what start leaves behind (the table kernels' d00)
// is the tile's, and frame may read it.
template <class Start, class Frame>
__device__ __forceinline__ void resample_tiles(const alac_resample_io& p, uint32_t a, uint32_t b, uint32_t N, uint32_t span, uint32_t num,
                                               float* xs, uint32_t group, uint32_t c, uint64_t row, const Start& start, const Frame& frame) {
    const resample_row r = resample_row_of(p, c, row, b);
    for (uint32_t t = 0; t < p.tiles_per_wg; ++t) {
        const uint64_t k0 = ((uint64_t)group * p.tiles_per_wg + t) * p.tile;
        if (k0 >= p.out_frames) break;
        const int64_t j0 = r.first + (int64_t)k0;
        const int64_t jn = j0 * (int64_t)num;
        int64_t q0 = jn / (int64_t)b;
        int64_t r0 = jn - q0 * (int64_t)b;
        if (r0 < 0) {
            r0 += (int64_t)b;
            q0 -= 1;
        }
        resample_stage(xs, span, start(q0, r0), r);
        const uint64_t left = p.out_frames - k0;
        const uint32_t n_out = left < p.tile ? (uint32_t)left : p.tile;
        for (uint32_t k = threadIdx.x; k < n_out; k += ALAC_RESAMPLE_THREADS) {
            uint32_t rel;
            auto weight = frame(r0, k, rel);
            rel = rel > span - N ? span - N : rel;            // (never, for a table that is what resample.py makes it and for a ratio)
            const float* const x = xs + rel;
            float acc = 0.0f;
            for (uint32_t n = 0; n < N; ++n) acc = __builtin_fmaf(weight(n), x[n], acc);
            const int64_t j = j0 + (int64_t)k;
            r.dst[k0 + k] = (j >= 0 && j * (int64_t)a < r.end_b) ? acc : 0.0f;
        }
    }
}

// The table kernels' tiles: the table into LDS in front of the span; frame j = i + b m reads from m a + d0[i] on (d0 is the
// caller's), and tap n weighs w[i][n]
__device__ __forceinline__ void table_tiles(const alac_resample_io& p, const resample_table_view& tb, float* lds, uint32_t group, uint32_t c,
                                            uint64_t row) {
    const uint32_t N = 2u * tb.width + 1u;
    const uint32_t table = tb.b * N;
    float* const w = lds;
    for (uint32_t i = threadIdx.x; i < table; i += ALAC_RESAMPLE_THREADS) w[i] = tb.weights[i];
    int32_t d00;
    resample_tiles(p, tb.a, tb.b, N, tb.span, 1u, lds + ((table + 3u) & ~3u), group, c, row,
                   [&](int64_t m0, int64_t i0) {
                       d00 = tb.d0[i0];
                       return m0 * (int64_t)tb.a + d00;
                   },
                   [&](int64_t i0, uint32_t k, uint32_t& rel) {
                       const uint32_t ii = (uint32_t)i0 + k;
                       const uint32_t mo = ii / tb.b;
                       const uint32_t i = ii - mo * tb.b;
                       rel = mo * tb.a + (uint32_t)(tb.d0[i] - d00);
                       const float* const wr = w + i * N;
                       return [wr](uint32_t n) { return wr[n]; };
                   });
}

}  // namespace

__global__ __launch_bounds__(ALAC_RESAMPLE_THREADS) void alac_resample_kernel(alac_resample_params p) {
    extern __shared__ __align__(16) float lds[];
    uint32_t group, c;
    uint64_t row;
    resample_place(p.io, group, c, row);
    table_tiles(p.io, {p.d0, p.weights, p.a, p.b, p.width, p.span}, lds, group, c, row);
}

__global__ __launch_bounds__(ALAC_RESAMPLE_THREADS) void alac_resample_rows_kernel(alac_resample_rows_params p) {
    extern __shared__ __align__(16) float lds[];
    uint32_t group, c;
    uint64_t row;
    resample_place(p.io, group, c, row);
    // the row's table: everything here is workgroup-uniform.  A descriptor that is not what the host was shown (no ratio, a
    // table or a span that does not fit the LDS of this launch) counts as no table: nothing is ever stored outside the LDS
    const uint32_t ti = p.row_table[row];
    bool has = ti < p.n_tables;
    resample_table_view t = {};
    if (has) {
        const alac_resample_table d = p.tables[ti];
        const uint64_t weights = (uint64_t)d.b * (2u * (uint64_t)d.width + 1u);
        has = d.a != 0 && d.b != 0 && d.width != 0 && weights <= ALAC_RESAMPLE_MAX_TABLE;
        if (has) {
            const uint64_t span = alac_resample_span(p.io.tile, d.a, d.b, d.width);
            has = ((weights + 3u) & ~3ull) + span <= p.lds_floats;
            t = {p.d0 + d.d0_first, p.weights + d.weights_first, d.a, d.b, d.width, (uint32_t)span};
        }
    }
    if (has) {
        table_tiles(p.io, t, lds, group, c, row);
        return;
    }
    // a row without a table (the crop of a file or an offset outside the corpus): zeros
    const uint32_t out_channels = p.io.mono ? 1u : p.io.channels;
    float* const dst = p.io.out + (row * out_channels + c) * p.io.out_frames;
    const uint64_t k0 = (uint64_t)group * p.io.tiles_per_wg * p.io.tile;
    const uint64_t left = p.io.out_frames > k0 ? p.io.out_frames - k0 : 0u;
    const uint64_t most = (uint64_t)p.io.tiles_per_wg * p.io.tile;
    const uint32_t n_out = (uint32_t)(left < most ? left : most);
    for (uint32_t k = threadIdx.x; k < n_out; k += ALAC_RESAMPLE_THREADS) dst[k0 + k] = 0.0f;
}

// ---- a ratio per row, the weights evaluated per tap (alacgpu_resample_ratio_rows_device) ---------------------------------------
// Speed perturbation makes ratios whose tables no LDS holds (44.1 kHz at factor 0.9 to 16 kHz is 3969 : 1600, 52800 weights),
// and a different one per row.  The filter is one function of one variable (alac.net_amd/speed.py states all of this operation
// by operation, and its numpy twin restates it): with M = max(a, b), the tap at source frame floor(j a / b) + d of output frame
// j, j a = q b + r, has
//     n = d b - r,   v = 99 n / (100 M),   weight = scale * sinc(v) * cos^2(pi v / 12) for |v| < 6, else 0,
// scale = 0.99 min(a, b) / a.  k = 99 n is an exact integer that grows by 99 b from tap to tap; so does its residue modulo the
// period 200 M of sin(pi v), with one conditional subtraction.  sin(pi |v|) is then +-sin(pi x), x = m / (100 M) in [0, 1/2]
// from an integer m, and cos(pi v / 12) is sin(pi x), x = (600 M - |k|) / (1200 M) in (0, 1/2]: both arguments are reduced
// before anything is rounded, and one odd polynomial of degree 13 serves both.  Nothing here is contracted, the division is the
// correctly rounded one, and no hardware transcendental is used.
//
// The workgroup is the table kernels': tiles of `tile` output frames of one (row, output channel), the tile's source span in
// LDS, a thread per output frame, N fused multiply-adds in ascending tap order, one writer per element.  The integers are 32
// bits wide where 1200 M and every k fit 31 bits (every audio ratio), else 64.
#pragma clang fp contract(off)

namespace {

// sin(pi x) for 0 <= x <= 1/2: the Taylor polynomial of degree 13, its coefficients (-1)^k pi^(2k+1) / (2k+1)! rounded to float32
__device__ __forceinline__ float ratio_sinpi(float x) {
    const float z = x * x;
    float p = 0x1.e8f434p-12f;
    p = __builtin_fmaf(p, z, -0x1.e3075p-8f);
    p = __builtin_fmaf(p, z, 0x1.507834p-4f);
    p = __builtin_fmaf(p, z, -0x1.32d2ccp-1f);
    p = __builtin_fmaf(p, z, 0x1.466bc6p+1f);
    p = __builtin_fmaf(p, z, -0x1.4abbcep+2f);
    p = __builtin_fmaf(p, z, 0x1.921fb6p+1f);
    return x * p;
}

// A row's ratio as the taps use it; I: int32_t or int64_t
template <class I>
struct ratio_view {
    I period, half, quarter;      // 200 M, 100 M, 50 M
    I reach;                      // 600 M: |k| at and above it is outside the filter
    I step;                       // 99 b
    float inv100, inv1200;        // 1 / float(100 M), 1 / float(1200 M)
    float scale;                  // float(99 min(a, b)) / float(100 a)
};

// The weight of the tap with k = 99 n and m = k mod 200 M (in 0 .. 200 M)
template <class I>
__device__ __forceinline__ float ratio_weight(const ratio_view<I>& r, I k, I m) {
    const I mag = k < 0 ? -k : k;
    I ms = (k < 0 && m != 0) ? r.period - m : m;            // |k| mod 200 M
    const bool minus = ms >= r.half;
    ms = minus ? ms - r.half : ms;
    ms = ms > r.quarter ? r.half - ms : ms;
    const float s = ratio_sinpi((float)ms * r.inv100);
    const float c = ratio_sinpi((float)(r.reach - mag) * r.inv1200);
    const float pv = ((float)mag * r.inv100) * 0x1.921fb6p+1f;
    const float g = ((minus ? -s : s) * (c * c)) / pv;
    const float w = mag == 0 ? r.scale : r.scale * g;
    return mag >= r.reach ? 0.0f : w;
}

// The ratio kernel's tiles: frame j, j a = q b + rem, reads from q - width on, and tap n weighs ratio_weight at k = 99 (n b -
// width b - rem), which grows by 99 b from tap to tap, its residue m with it
template <class I>
__device__ __forceinline__ void ratio_tiles(const alac_resample_io& p, const alac_resample_ratio d, uint32_t span, float* xs, uint32_t group,
                                            uint32_t c, uint64_t row) {
    typedef typename std::conditional<sizeof(I) == 4, uint32_t, uint64_t>::type U;
    const uint64_t M = d.a > d.b ? d.a : d.b;
    ratio_view<I> r;
    r.period = (I)(200u * M);
    r.half = (I)(100u * M);
    r.quarter = (I)(50u * M);
    r.reach = (I)(600u * M);
    r.step = (I)(99u * (uint64_t)d.b);
    r.inv100 = 1.0f / (float)(int64_t)(100u * M);
    r.inv1200 = 1.0f / (float)(int64_t)(1200u * M);
    r.scale = (float)(int64_t)(99u * (uint64_t)(d.a < d.b ? d.a : d.b)) / (float)(int64_t)(100u * (uint64_t)d.a);
    resample_tiles(p, d.a, d.b, 2u * d.width + 1u, span, d.a, xs, group, c, row,
                   [&](int64_t q0, int64_t r0) { return q0 - (int64_t)d.width; },
                   [&](int64_t r0, uint32_t k, uint32_t& rel) {
                       // frame j0 + k: (j0 + k) a = (q0 + q) b + rem -- its taps are xs[q ..+ N], the first one d = -width
                       const U ta = (U)r0 + (U)k * (U)d.a;
                       const U q = ta / (U)d.b;
                       const U rem = ta - q * (U)d.b;
                       rel = (uint32_t)q;
                       const U below = (U)99u * ((U)d.width * (U)d.b + rem);     // -k of the first tap, above 0
                       const U mm = below % (U)r.period;
                       I kk = -(I)below;
                       I m = mm ? r.period - (I)mm : (I)0;
                       return [&r, kk, m](uint32_t n) mutable {
                           const float w = ratio_weight(r, kk, m);
                           kk += r.step;
                           m += r.step;
                           m = m >= r.period ? m - r.period : m;
                           return w;
                       };
                   });
}

}  // namespace

__global__ __launch_bounds__(ALAC_RESAMPLE_THREADS) void alac_resample_ratio_rows_kernel(alac_resample_ratio_params p) {
    extern __shared__ __align__(16) float lds[];
    uint32_t group, c;
    uint64_t row;
    resample_place(p.io, group, c, row);
    // the row's ratio: workgroup-uniform.  A row that names none, a ratio with a == 0, and a descriptor that is not what the
    // host was shown (a span that does not fit the LDS of this launch) are skipped: the row's output stays as it is
    const uint32_t ri = p.row_ratio[row];
    if (ri >= p.n_ratios) return;
    const alac_resample_ratio d = p.ratios[ri];
    if (d.a == 0 || d.b == 0 || d.width == 0 || d.width > ALAC_RESAMPLE_RATIO_MAX_WIDTH || (d.a | d.b) >> 31) return;
    const uint64_t span = alac_resample_span(p.io.tile, d.a, d.b, d.width);
    if (span > p.lds_floats) return;
    // 32-bit integers where 1200 M, the first tap's 99 (width b + b) and a tile's r0 + (tile - 1) a all stay below 2^31
    const uint64_t M = d.a > d.b ? d.a : d.b;
    const uint64_t most = 99u * ((uint64_t)d.width + 2u) * d.b;
    if (1200u * M < (1ull << 31) && most < (1ull << 31) && (uint64_t)p.io.tile * d.a + d.b < (1ull << 31))
        ratio_tiles<int32_t>(p.io, d, (uint32_t)span, lds, group, c, row);
    else
        ratio_tiles<int64_t>(p.io, d, (uint32_t)span, lds, group, c, row);
}
