// alac_level.hip -- peak, RMS and BS.1770 loudness levelling of the crops, behind the noise mix and in front of the biquad
// cascade: two launches, no atomics, nothing read back.  include/alacgpu.h states the arithmetic, alac_level.h the blocking and
// the order of every sum, alac.net_amd/level.py every operation in order.  Everything is float64, one IEEE operation at a time
// through __dmul_rn / __dadd_rn / __ddiv_rn / __dsqrt_rn, nothing contracted (alac_biquad_tile.h switches it off), and the
// kernels evaluate no logarithm and no power: the targets and the gate are linear numbers.  src and out may be the same array:
// the measure launch only reads, and the apply launch stores what the same lane loaded.
#include "alac_level.h"
#include "alac_biquad_tile.h"

using namespace alac_biquad_tile;

namespace {

constexpr uint32_t THREADS = ALAC_LEVEL_THREADS;

__device__ inline double quot(double a, double b) { return __ddiv_rn(a, b); }

// the larger of two magnitudes; a NaN on either side stays
__device__ inline double larger(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ inline uint64_t valid_frames(const alac_level_params& p, uint32_t row) {
    if (!p.valid) return p.frames;
    const int64_t a = p.valid[row];
    return a <= 0 ? 0u : ((uint64_t)a < p.frames ? (uint64_t)a : p.frames);
}

struct measure_lds {
    double tab[2 * ALAC_BIQUAD_TAB];
    state hist[2 * THREADS];
    state wtot[2 * WAVES];
    state carry[2 * ALAC_BIQUAD_MAX_SECTIONS];
    double first[THREADS], second[THREADS];       // a chunk's partials of the two hops it touches
    double open_hop[2];                           // the sum of the hop that runs on into the next tile, by the tile's parity
    double wsum[2 * WAVES], wpeak[2 * WAVES];
};

template <bool LUFS, bool VEC>
__device__ inline void measure_plane(const alac_level_params& p, const float* x, uint64_t v, double* s, measure_lds& m) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t hop = p.hop;
    const uint64_t lim = LUFS ? v / hop * hop : 0u;       // the frames of the whole hops
    double total = 0.0, peak = 0.0;                       // (lane 0's)
    uint32_t par = 0;
    for (uint64_t t0 = 0; t0 < v; t0 += ALAC_BIQUAD_TILE, par ^= 1u) {
        const uint64_t n0 = t0 + (uint64_t)CHUNK * tid;
        double u[CHUNK];
        load_chunk<VEC>(x, n0, v, u);
        double ps = 0.0, pk = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < CHUNK; j++) {
            ps = add(ps, mul(u[j], u[j]));
            pk = larger(pk, fabs(u[j]));
        }
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
            ps = add(ps, __shfl_down(ps, h, 64));
            pk = larger(pk, __shfl_down(pk, h, 64));
        }
        if (lane == 0u) m.wsum[par * WAVES + wave] = ps, m.wpeak[par * WAVES + wave] = pk;
        if (LUFS) {
            run_sections(u, 2u, t0, par, m.tab, m.hist, m.wtot, m.carry);
            double a = 0.0, b = 0.0;
            if (n0 < lim) {
                const uint64_t bnd = (n0 / hop + 1u) * hop;           // behind the hop of the chunk's first frame
#pragma unroll
                for (uint32_t j = 0; j < CHUNK; j++) {
                    const uint64_t n = n0 + j;
                    const double q = mul(u[j], u[j]);
                    if (n < bnd) a = add(a, q);
                    else if (n < lim) b = add(b, q);
                }
            }
            m.first[tid] = a;
            m.second[tid] = b;
        }
        __syncthreads();
        if (tid == 0u) {
            const double* const w = m.wsum + par * WAVES;
            const double* const k = m.wpeak + par * WAVES;
            total = add(total, add(add(w[0], w[2]), add(w[1], w[3])));
            peak = larger(larger(peak, larger(k[0], k[2])), larger(k[1], k[3]));
        }
        const uint64_t end = t0 + ALAC_BIQUAD_TILE < lim ? t0 + ALAC_BIQUAD_TILE : lim;
        if (LUFS && end > t0) {
            // every hop that has frames in this tile, a lane each: the partials of its chunks in ascending order
            const uint64_t klast = (end - 1u) / hop;
            for (uint64_t k = t0 / hop + tid; k <= klast; k += THREADS) {
                const uint64_t hs = k * hop, he = hs + hop;
                const uint64_t f0 = hs > t0 ? hs : t0, f1 = he < end ? he : end;
                const uint32_t l0 = (uint32_t)(f0 - t0) / CHUNK, l1 = (uint32_t)(f1 - 1u - t0) / CHUNK;
                double acc = hs < t0 ? m.open_hop[par ^ 1u] : 0.0;
                for (uint32_t l = l0; l <= l1; l++) acc = add(acc, t0 + (uint64_t)CHUNK * l >= hs ? m.first[l] : m.second[l]);
                if (he <= t0 + ALAC_BIQUAD_TILE) s[ALAC_LEVEL_HEAD + k] = acc;
                else m.open_hop[par] = acc;
            }
        }
    }
    if (tid == 0u) s[0] = total, s[1] = peak;
}

}  // namespace

// One (row, channel) a workgroup: its sum of squares, its peak and, for lufs, the sums of the squares of the K-weighted
// channel over every whole hop, into the plane's scratch.  A row with v == 0 leaves (0, 0).
__global__ __launch_bounds__(ALAC_LEVEL_THREADS) void alac_level_measure_kernel(alac_level_params p) {
    __shared__ measure_lds m;
    const uint32_t row = blockIdx.x / p.channels;
    const uint64_t v = valid_frames(p, row);
    double* const s = p.scratch + (uint64_t)blockIdx.x * (ALAC_LEVEL_HEAD + p.hops);
    if (v == 0u) {                                        // (the row's: every lane returns or none)
        if (threadIdx.x == 0u) s[0] = 0.0, s[1] = 0.0;
        return;
    }
    const float* const x = p.src + (uint64_t)blockIdx.x * p.stride;
    if (p.mode == ALAC_LEVEL_LUFS) {
        if (threadIdx.x < 2u) make_table(p.kweight + 5u * threadIdx.x, m.tab + threadIdx.x * ALAC_BIQUAD_TAB);
        __syncthreads();
        if (p.vec) measure_plane<true, true>(p, x, v, s, m);
        else measure_plane<true, false>(p, x, v, s, m);
    } else {
        if (p.vec) measure_plane<false, true>(p, x, v, s, m);
        else measure_plane<false, false>(p, x, v, s, m);
    }
}

// A part of a row a workgroup: the row's gain from its scratch (every workgroup of the row for itself, in the same order),
// then g x over the part's frames below v of every channel.
__global__ __launch_bounds__(ALAC_LEVEL_THREADS) void alac_level_apply_kernel(alac_level_params p) {
    __shared__ double eb[ALAC_LEVEL_BATCH];
    __shared__ double sh_thr, sh_g;
    __shared__ uint32_t sh_write;
    const uint32_t tid = threadIdx.x, row = blockIdx.x / p.parts, part = blockIdx.x % p.parts, C = p.channels;
    const uint64_t v = valid_frames(p, row);
    const uint64_t plane = ALAC_LEVEL_HEAD + p.hops;
    const double* const s = p.scratch + (uint64_t)row * C * plane;
    const bool lufs = p.mode == ALAC_LEVEL_LUFS;
    const uint64_t nh = lufs ? v / p.hop : 0u, nb = nh >= 4u ? nh - 3u : 0u;
    const double span = (double)(4ull * p.hop);
    double sum[2] = {0.0, 0.0};
    uint64_t count[2] = {0u, 0u};                         // (lane 0's: the blocks above the absolute gate, above both)
    for (uint32_t pass = 0; pass < 2u; pass++) {
        const double thr = pass ? sh_thr : 0.0;
        for (uint64_t j0 = 0; j0 < nb; j0 += ALAC_LEVEL_BATCH) {
            const uint64_t j = j0 + tid;
            if (j < nb) {
                double e = 0.0;
                for (uint32_t c = 0; c < C; c++) {
                    const double* const h = s + c * plane + ALAC_LEVEL_HEAD + j;
                    const double z = quot(add(add(h[0], h[1]), add(h[2], h[3])), span);
                    const double w = mul(c < 3u ? ALAC_LEVEL_WEIGHT_FRONT : ALAC_LEVEL_WEIGHT_SURROUND, z);
                    e = c ? add(e, w) : w;
                }
                eb[tid] = e;
            }
            __syncthreads();
            if (tid == 0u) {
                const uint32_t n = nb - j0 < ALAC_LEVEL_BATCH ? (uint32_t)(nb - j0) : ALAC_LEVEL_BATCH;
                for (uint32_t i = 0; i < n; i++) {
                    const double e = eb[i];
                    if (e > ALAC_LEVEL_GATE_ABS && (!pass || e > thr)) sum[pass] = add(sum[pass], e), count[pass]++;
                }
            }
            __syncthreads();
        }
        if (!pass) {
            if (tid == 0u) sh_thr = mul(ALAC_LEVEL_GATE_REL, quot(sum[0], (double)count[0]));      // (no block: a NaN, nothing is above it)
            __syncthreads();
        }
    }
    if (tid == 0u) {
        double P = 0.0, S = 0.0;
        for (uint32_t c = 0; c < C; c++) {
            S = c ? add(S, s[c * plane]) : s[0];
            P = larger(P, s[c * plane + 1u]);
        }
        bool measured = v != 0u && P != 0.0;
        double E = 0.0, g = 1.0;
        if (measured) {
            if (lufs) {
                measured = count[0] != 0u;
                if (measured) E = quot(sum[1], (double)count[1]);
            } else {
                E = quot(S, (double)((uint64_t)C * v));
            }
            measured = measured && E != 0.0;
        }
        if (measured) {
            g = p.mode == ALAC_LEVEL_PEAK ? quot(p.target, P) : __dsqrt_rn(quot(p.target, E));
            if (p.max_peak > 0.0) {
                const double most = quot(p.max_peak, P);
                if (most < g) g = most;
            }
        }
        if (part == 0u) {
            if (p.gain_out) p.gain_out[row] = g;
            if (p.energy_out) p.energy_out[row] = E;
            if (p.peak_out) p.peak_out[row] = P;
        }
        sh_g = g;
        sh_write = measured && p.out && (g != 1.0 || p.clamp) ? 1u : 0u;
    }
    __syncthreads();
    if (!sh_write) return;                                // (the row's: every lane returns or none)
    const double g = sh_g;
    const uint64_t f0 = (uint64_t)part * p.part_frames;
    const uint64_t f1 = f0 + p.part_frames < v ? f0 + p.part_frames : v;
    if (f0 >= f1) return;
    const auto scaled = [&](float a) {
        float r = (float)mul(g, (double)a);
        if (p.clamp) r = r < -1.0f ? -1.0f : (r > 1.0f ? 1.0f : r);          // (a NaN stays one)
        return r;
    };
    for (uint32_t c = 0; c < C; c++) {
        const float* const x = p.src + ((uint64_t)row * C + c) * p.stride;
        float* const y = p.out + ((uint64_t)row * C + c) * p.stride;
        uint64_t done = f0;
        if (p.vec_out) {
            done = f0 + ((f1 - f0) & ~3ull);
            for (uint64_t i = f0 + 4ull * tid; i < done; i += 4ull * THREADS) {
                const float4 a = *reinterpret_cast<const float4*>(x + i);
                *reinterpret_cast<float4*>(y + i) = make_float4(scaled(a.x), scaled(a.y), scaled(a.z), scaled(a.w));
            }
        }
        for (uint64_t i = done + tid; i < f1; i += THREADS) y[i] = scaled(x[i]);
    }
}
