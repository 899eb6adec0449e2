// alac_biquad.hip -- a cascade of biquad sections and a gain per row on the waveform, between the noise mix and the features:
// one launch, no atomics, no scratch.  include/alacgpu.h states the arithmetic, alac_biquad.h the blocking, alac.net_amd/biquad.py
// every operation in order.  The recurrences are float64: every operation is one IEEE float64 operation, rounded once -- this
// file is compiled with -ffp-contract=off and the products and sums go through __dmul_rn / __dadd_rn / __dsub_rn, so no multiply
// is fused into an add and the twin needs no float64 FMA.  src and out may be the same array: a lane stores the frames it
// loaded itself, and no other lane reads them.
#include "alac_biquad.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t CHUNK = ALAC_BIQUAD_CHUNK, LEVELS = ALAC_BIQUAD_LEVELS, WAVES = ALAC_BIQUAD_THREADS / 64;

__device__ inline double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ inline double add(double a, double b) { return __dadd_rn(a, b); }
__device__ inline double sub(double a, double b) { return __dsub_rn(a, b); }

struct state {
    double x, y;                  // (y[n-1], y[n-2])
};

// P t: ((p00 t0) + (p01 t1), (p10 t0) + (p11 t1)), P = (p00, p01, p10, p11)
__device__ inline state apply(const double* P, state t) {
    return {add(mul(P[0], t.x), mul(P[1], t.y)), add(mul(P[2], t.x), mul(P[3], t.y))};
}

__device__ inline state plus(state a, state b) { return {add(a.x, b.x), add(a.y, b.y)}; }

__device__ inline state lane_below(state s, int d) { return {__shfl_up(s.x, d, 64), __shfl_up(s.y, d, 64)}; }

// A section's table from its coefficients: the two homogeneous responses over a chunk by running the recurrence, M from their
// last two values, its powers by squaring.  One lane, once per row.
__device__ inline void make_table(const double* q, double* tab) {
#pragma unroll
    for (uint32_t i = 0; i < 5u; i++) tab[i] = q[i];
    const double a1 = q[3], a2 = q[4];
    double* const h = tab + ALAC_BIQUAD_TAB_H;
#pragma unroll
    for (uint32_t r = 0; r < 2u; r++) {
        double p1 = r == 0u ? 1.0 : 0.0, p2 = r == 0u ? 0.0 : 1.0;
        for (uint32_t j = 0; j < CHUNK; j++) {
            const double g = sub(-mul(a1, p1), mul(a2, p2));
            p2 = p1;
            p1 = g;
            h[r * CHUNK + j] = g;
        }
    }
    double* P = tab + ALAC_BIQUAD_TAB_P;
    P[0] = h[CHUNK - 1u], P[1] = h[2u * CHUNK - 1u], P[2] = h[CHUNK - 2u], P[3] = h[2u * CHUNK - 2u];
    for (uint32_t i = 0; i < LEVELS; i++, P += 4) {
        P[4] = add(mul(P[0], P[0]), mul(P[1], P[2]));
        P[5] = add(mul(P[0], P[1]), mul(P[1], P[3]));
        P[6] = add(mul(P[2], P[0]), mul(P[3], P[2]));
        P[7] = add(mul(P[2], P[1]), mul(P[3], P[3]));
    }
}

template <bool VEC>
__device__ inline void biquad_plane(const alac_biquad_params& p, const float* x, float* y, uint64_t v, double g, const double* tab,
                                    state* hist, state* wtot, state* carry) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t S = p.sections;
    uint32_t par = 0;                                     // the tile's parity: which half of hist and carry it writes
    for (uint64_t t0 = 0; t0 < v; t0 += ALAC_BIQUAD_TILE, par ^= 1u) {
        const uint64_t n0 = t0 + (uint64_t)CHUNK * tid;
        const bool whole = VEC && n0 + CHUNK <= v;
        double u[CHUNK];
        if (whole) {
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j += 4u) {
                const float4 a = *reinterpret_cast<const float4*>(x + n0 + j);
                u[j] = a.x, u[j + 1] = a.y, u[j + 2] = a.z, u[j + 3] = a.w;
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j++) u[j] = n0 + j < v ? (double)x[n0 + j] : 0.0;      // (behind v: not read)
        }
        // the input's last two frames in front of every lane; in front of lane 0 the tile before's, zeros in front of the row
        hist[par * ALAC_BIQUAD_THREADS + tid] = {u[CHUNK - 1u], u[CHUNK - 2u]};
        __syncthreads();
        state in = {0.0, 0.0};
        if (tid) in = hist[par * ALAC_BIQUAD_THREADS + tid - 1u];
        else if (t0) in = hist[(par ^ 1u) * ALAC_BIQUAD_THREADS + ALAC_BIQUAD_THREADS - 1u];
        for (uint32_t k = 0; k < S; k++) {
            const double* const T = tab + k * ALAC_BIQUAD_TAB;
            const double b0 = T[0], b1 = T[1], b2 = T[2], a1 = T[3], a2 = T[4];
            // the FIR part, in place from the chunk's end
#pragma unroll
            for (uint32_t j = CHUNK - 1u; j >= 2u; j--) u[j] = add(add(mul(b0, u[j]), mul(b1, u[j - 1u])), mul(b2, u[j - 2u]));
            u[1] = add(add(mul(b0, u[1]), mul(b1, u[0])), mul(b2, in.x));
            u[0] = add(add(mul(b0, u[0]), mul(b1, in.x)), mul(b2, in.y));
            // the zero-state recursion
            double y1 = 0.0, y2 = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j++) {
                const double r = sub(sub(u[j], mul(a1, y1)), mul(a2, y2));
                u[j] = r;
                y2 = y1;
                y1 = r;
            }
            // the chunk-end states, scanned within the wave
            state s = {y1, y2};
            const double* const P = T + ALAC_BIQUAD_TAB_P;
#pragma unroll
            for (uint32_t i = 0; i < LEVELS; i++) {
                const state r = plus(apply(P + 4u * i, lane_below(s, 1 << i)), s);
                if (lane >= (1u << i)) s = r;
            }
            state* const wt = wtot + (k & 1u) * WAVES;
            if (lane == 63u) wt[wave] = s;
            __syncthreads();
            // the state in front of every wave, from the state the tile before left; every lane walks all waves
            state c = {0.0, 0.0}, cw = {0.0, 0.0};
            if (t0) c = carry[par * ALAC_BIQUAD_MAX_SECTIONS + k];
#pragma unroll
            for (uint32_t w = 0; w < WAVES; w++) {
                if (w == wave) cw = c;
                c = plus(apply(P + 4u * LEVELS, c), wt[w]);
            }
            if (tid == 0u) carry[(par ^ 1u) * ALAC_BIQUAD_MAX_SECTIONS + k] = c;
            // M^lane c_w, then the scan's value of the lane below: the state in front of this lane's chunk
            state e = cw;
#pragma unroll
            for (uint32_t i = 0; i < LEVELS; i++) {
                const state r = apply(P + 4u * i, e);
                if ((lane >> i) & 1u) e = r;
            }
            const state below = plus(e, lane_below(s, 1));
            if (lane) e = below;
            const double* const h1 = T + ALAC_BIQUAD_TAB_H;
            const double* const h2 = h1 + CHUNK;
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j++) u[j] = add(add(u[j], mul(h1[j], e.x)), mul(h2[j], e.y));
            in = e;                                       // the next section's input in front of the chunk
        }
        float r[CHUNK];
#pragma unroll
        for (uint32_t j = 0; j < CHUNK; j++) {
            float a = (float)mul(g, u[j]);
            if (p.clamp) a = a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);          // (a NaN stays one)
            r[j] = a;
        }
        if (whole) {
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j += 4u) *reinterpret_cast<float4*>(y + n0 + j) = make_float4(r[j], r[j + 1], r[j + 2], r[j + 3]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < CHUNK; j++)
                if (n0 + j < v) y[n0 + j] = r[j];
        }
    }
}

}  // namespace

// One (row, channel) a workgroup.  A row with v == 0, and a row whose sections are all (1, 0, 0, 0, 0) with a gain of 1 and no
// clamp, is neither read nor written.
__global__ __launch_bounds__(ALAC_BIQUAD_THREADS) void alac_biquad_kernel(alac_biquad_params p) {
    __shared__ double tab[ALAC_BIQUAD_MAX_SECTIONS * ALAC_BIQUAD_TAB];
    __shared__ state hist[2 * ALAC_BIQUAD_THREADS];
    __shared__ state wtot[2 * WAVES];
    __shared__ state carry[2 * ALAC_BIQUAD_MAX_SECTIONS];
    const uint32_t row = blockIdx.x / p.channels;
    uint64_t v = p.frames;
    if (p.valid) {
        const int64_t a = p.valid[row];
        v = a <= 0 ? 0u : ((uint64_t)a < p.frames ? (uint64_t)a : p.frames);
    }
    if (v == 0u) return;                                  // (the row's: every lane returns or none)
    const double* const q = p.coeffs + (uint64_t)row * p.sections * 5u;
    const double g = p.gain ? p.gain[row] : 1.0;
    bool identity = g == 1.0 && !p.clamp;
    for (uint32_t k = 0; k < p.sections; k++)
        identity = identity && q[5u * k] == 1.0 && q[5u * k + 1u] == 0.0 && q[5u * k + 2u] == 0.0 && q[5u * k + 3u] == 0.0 &&
                   q[5u * k + 4u] == 0.0;
    if (identity) return;
    if (threadIdx.x < p.sections) make_table(q + 5u * threadIdx.x, tab + threadIdx.x * ALAC_BIQUAD_TAB);
    __syncthreads();
    const float* const x = p.src + (uint64_t)blockIdx.x * p.stride;
    float* const y = p.out + (uint64_t)blockIdx.x * p.stride;
    if (p.vec) biquad_plane<true>(p, x, y, v, g, tab, hist, wtot, carry);
    else biquad_plane<false>(p, x, y, v, g, tab, hist, wtot, carry);
}
