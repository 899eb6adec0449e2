// alac_biquad_tile.h -- the tile body of the blocked float64 biquad recurrence as __device__ functions, for the kernels that run
// it: alac_biquad.hip stores the result, alac_level.hip squares it into its hop sums.  alac_biquad.h states the blocking,
// alac.net_amd/biquad.py every operation in order.  Every operation is one IEEE float64 operation, rounded once: the products
// and sums go through __dmul_rn / __dadd_rn / __dsub_rn and contraction is off from here to the end of the including file, so
// no multiply is fused into an add and the twin needs no float64 FMA.
#pragma once
#include "alac_biquad.h"

#pragma clang fp contract(off)

namespace alac_biquad_tile {

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

// The lane's chunk of the tile at t0, frames n0 = t0 + CHUNK * lane on, widened to float64; a frame at or behind v is not read
// and counts as 0.  True: the chunk lies below v and was read with 16-byte loads (it may then be stored that way).
template <bool VEC>
__device__ inline bool load_chunk(const float* x, uint64_t n0, uint64_t v, double* u) {
    const bool whole = VEC && n0 + CHUNK <= v;
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
    return whole;
}

// The tile's chunks u (as loaded) through the S sections of tab, in place: every lane of the workgroup calls it for every
// tile of the plane in ascending order, t0 the tile's first frame and par its parity (which half of hist and carry it
// writes).  hist: 2 * ALAC_BIQUAD_THREADS, wtot: 2 * WAVES, carry: 2 * ALAC_BIQUAD_MAX_SECTIONS states of LDS.
__device__ inline void run_sections(double* u, uint32_t S, uint64_t t0, uint32_t par, const double* tab, state* hist, state* wtot,
                                    state* carry) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
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
}

}  // namespace alac_biquad_tile
