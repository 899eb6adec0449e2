// alac_pyin.hip -- probabilistic YIN behind the crops (Mauch and Dixon 2014), two launches: the observation of every frame and
// the Viterbi decode along every plane.  alac_pyin.h states the parameters and the LDS images, alac.net_amd/pyin.py every
// operation in order.  All float32, one IEEE operation at a time: this file is compiled with -ffp-contract=off and
// -fhip-fp32-correctly-rounded-divide-sqrt, sums, differences and products go through __fadd_rn / __fsub_rn / __fmul_rn, and the
// logarithm is alac_pcen.h's explicit polynomial.  Every tie goes to the lowest source state: a candidate replaces the best so
// far only when it is strictly larger, and candidates come in ascending order.  Plain vector stores only, no atomics.
#include "alac_pcen.h"
#include "alac_pyin.h"
#include "alac_yin_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr float PYIN_FLOOR = 1.17549435e-38f;                      // 2^-126

__device__ inline float pyin_log2_floor(float p) { return alac_pcen_log2(p < PYIN_FLOOR ? PYIN_FLOOR : p); }

// m of a height: the number of thresholds s_i with not (h < s_i); s ascends, h is no NaN
__device__ inline uint32_t pyin_thresholds_under(const float* s, uint32_t N, float h) {
    uint32_t lo = 0u, hi = N;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (h < s[mid]) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// The bin of a period: the number of edges with period < edge; the edges descend
__device__ inline uint32_t pyin_bin(const float* edges, uint32_t n_edges, float period) {
    uint32_t lo = 0u, hi = n_edges;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (period < edges[mid]) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// Steps 2 to 6 of one frame by one wave, d' [tau_max + 1] in LDS: the troughs by ballot in chunks of 64 lags, twice.  The first
// pass counts, per threshold of the lane, the troughs below it (n_i) and finds the first trough of the least height; the
// second visits the troughs again in ascending order with a running count per threshold (pos_i(k)), reduces P_k in the order
// pyin.py states (a lane's thresholds ascending, then the tree of halves over the lanes) and lets lane 0 add it to its bin.
__device__ inline void pyin_frame(const alac_pyin_obs_params& q, const float* d, const float* bz, const float* inv, float* acc,
                                  uint32_t lane, float* ov, float* ou, float* vp_out) {
    const uint32_t last = q.y.tau_max - 1u, N = q.n_thresholds, n_bins = q.n_bins;
    for (uint32_t b = lane; b < n_bins; b += 64u) acc[b] = 0.0f;
    wave_sync();
    float beta[ALAC_PYIN_LANE_THRESHOLDS];
    uint32_t total[ALAC_PYIN_LANE_THRESHOLDS], seen[ALAC_PYIN_LANE_THRESHOLDS];
#pragma unroll
    for (uint32_t j = 0; j < ALAC_PYIN_LANE_THRESHOLDS; j++) {
        const uint32_t i = lane + 1u + 64u * j;                    // (the threshold, from 1)
        beta[j] = i <= N ? q.tab.beta[i - 1u] : 0.0f;
        total[j] = seen[j] = 0u;
    }
    float least = __builtin_inff();
    uint32_t k_least = 0xFFFFFFFFu, k = 0u;
    for (uint32_t base = q.y.tau_min; base <= last; base += 64u) {
        const uint32_t t = base + lane;
        const bool is = t <= last && d[t] < d[t - 1u] && d[t] <= d[t + 1u];
        unsigned long long hit = __ballot(is);
        const float h = is ? d[t] : 0.0f;
        const uint32_t m = is ? pyin_thresholds_under(q.tab.s, N, h) : 0u;
        while (hit) {
            const int from = __builtin_ctzll(hit);
            hit &= hit - 1ull;
            const uint32_t mk = (uint32_t)__shfl((int)m, from, 64);
            const float hk = __shfl(h, from, 64);
#pragma unroll
            for (uint32_t j = 0; j < ALAC_PYIN_LANE_THRESHOLDS; j++)
                if (mk < lane + 1u + 64u * j) total[j]++;
            if (hk < least) least = hk, k_least = k;
            k++;
        }
    }
    float v = 0.0f;
    k = 0u;
    for (uint32_t base = q.y.tau_min; base <= last; base += 64u) {
        const uint32_t t = base + lane;
        const bool is = t <= last && d[t] < d[t - 1u] && d[t] <= d[t + 1u];
        unsigned long long hit = __ballot(is);
        uint32_t m = 0u, bin = 0u;
        if (is) {
            const float a = d[t - 1u], b = d[t], c = d[t + 1u];
            m = pyin_thresholds_under(q.tab.s, N, b);
            const float n = __fsub_rn(a, c), den = __fadd_rn(__fsub_rn(a, __fmul_rn(2.0f, b)), c);
            const float shift = (b <= a && b <= c && den > 0.0f) ? __fmul_rn(0.5f, n) / den : 0.0f;
            bin = pyin_bin(q.tab.edges, n_bins - 1u, __fadd_rn((float)t, shift));
        }
        while (hit) {
            const int from = __builtin_ctzll(hit);
            hit &= hit - 1ull;
            const uint32_t mk = (uint32_t)__shfl((int)m, from, 64), at = (uint32_t)__shfl((int)bin, from, 64);
            float part = 0.0f;
#pragma unroll
            for (uint32_t j = 0; j < ALAC_PYIN_LANE_THRESHOLDS; j++) {
                const uint32_t i = lane + 1u + 64u * j;
                if (i <= N && mk < i) {
                    part = __fadd_rn(part, __fmul_rn(__fmul_rn(beta[j], bz[seen[j]]), inv[total[j]]));
                    seen[j]++;
                }
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) part = __fadd_rn(part, __shfl_xor(part, w, 64));
            if (k == k_least) part = __fadd_rn(part, __fmul_rn(q.no_trough, q.tab.cb[mk]));
            if (lane == 0u) acc[at] = __fadd_rn(acc[at], part);
            v = __fadd_rn(v, part);
            k++;
        }
    }
    wave_sync();
    const float vp = v < 1.0f ? v : 1.0f;
    for (uint32_t b = lane; b < n_bins; b += 64u) ov[b] = pyin_log2_floor(acc[b]);
    if (lane == 0u) {
        *ou = pyin_log2_floor(__fsub_rn(1.0f, vp) / (float)n_bins);
        *vp_out = vp;
    }
}

template <bool VEC>
__device__ inline void pyin_obs_tile(const alac_pyin_obs_params& q, float* lds) {
    const alac_yin_params& p = q.y;
    const yin_tile_at at = yin_tile_where(p);
    const uint32_t tid = threadIdx.x, n_bins = q.n_bins, nf = at.nf;
    float* ov = q.obs_voiced + (uint64_t)at.plane * p.out_frames * n_bins;
    float* ou = q.obs_unvoiced + (uint64_t)at.plane * p.out_frames;
    float* vp = q.vp + (uint64_t)at.plane * p.out_frames;
    // the frames of the tile at and behind the row's count: zeros
    for (uint32_t f = nf; f < p.tile; f++) {
        const uint64_t t = at.t0 + f;
        if (t >= p.out_frames) break;
        for (uint32_t b = tid; b < n_bins; b += ALAC_YIN_THREADS) ov[t * n_bins + b] = 0.0f;
        if (tid == 0u) ou[t] = 0.0f, vp[t] = 0.0f;
    }
    if (nf == 0u) return;                                          // (the whole workgroup, before any load)
    const uint32_t lags = p.tau_max + 1u, K1 = q.max_troughs + 1u;
    float* bz = lds + p.samples + (size_t)p.tile * lags;
    float* inv = bz + K1;
    for (uint32_t i = tid; i < K1; i += ALAC_YIN_THREADS) bz[i] = q.tab.bz[i], inv[i] = q.tab.inv[i];
    float* dd = yin_tile_difference<VEC>(p, lds, at);            // (its barriers stand behind the two tables too)
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    float* acc = inv + K1 + (size_t)wave * n_bins;
    for (uint32_t f = wave; f < nf; f += ALAC_YIN_THREADS / 64) {
        float* d = dd + (size_t)f * lags;
        (void)yin_dprime(p.tau_max, d, lane);                      // (silence: d' is 1 everywhere and has no trough)
        const uint64_t t = at.t0 + f;
        pyin_frame(q, d, bz, inv, acc, lane, ov + t * n_bins, ou + t, vp + t);
        wave_sync();                                               // (acc is the next frame's)
    }
}

}  // namespace

__global__ __launch_bounds__(ALAC_YIN_THREADS) void alac_pyin_obs_kernel(alac_pyin_obs_params p) {
    extern __shared__ __align__(16) float pyin_lds[];
    pyin_obs_tile<false>(p, pyin_lds);
}

// hop % 4 == 0: every frame starts on a 16-byte boundary of the LDS image
__global__ __launch_bounds__(ALAC_YIN_THREADS) void alac_pyin_obs_kernel_vec(alac_pyin_obs_params p) {
    extern __shared__ __align__(16) float pyin_lds[];
    pyin_obs_tile<true>(p, pyin_lds);
}

__global__ __launch_bounds__(ALAC_PYIN_DECODE_THREADS) void alac_pyin_decode_kernel(alac_pyin_decode_params p) {
    __shared__ float e_lds[2][2u * ALAC_PYIN_MAX_BINS];            // delta - lz of both halves, double-buffered
    __shared__ float delta_lds[2u * ALAC_PYIN_MAX_BINS];           // the last frame's delta
    __shared__ float lt_lds[ALAC_PYIN_MAX_BINS], lz_lds[ALAC_PYIN_MAX_BINS];
    __shared__ float best_lds[ALAC_PYIN_DECODE_THREADS / 64];
    __shared__ uint32_t at_lds[ALAC_PYIN_DECODE_THREADS / 64];
    const uint32_t plane = blockIdx.x, row = plane / p.channels, tid = threadIdx.x;
    const uint32_t n = p.n_bins, S = 2u * n, band = p.band;
    const uint64_t F = p.out_frames;
    uint64_t count = F;
    if (p.counts_are_frames) {
        if (p.valid) {
            const int64_t a = p.valid[row];
            count = a <= 0 ? 0u : ((uint64_t)a < F ? (uint64_t)a : F);
        }
    } else {
        uint64_t v = p.frames;
        if (p.valid) {
            const int64_t a = p.valid[row];
            v = a <= 0 ? 0u : ((uint64_t)a < p.frames ? (uint64_t)a : p.frames);
        }
        count = p.align ? (v < p.align ? 0u : 1u + (v - p.align) / p.hop) : v / p.hop + 1u;
        if (count > F) count = F;
    }
    float* out = p.out ? p.out + (uint64_t)plane * 3u * F : nullptr;
    int32_t* states = p.states ? p.states + (uint64_t)plane * F : nullptr;
    // at and behind the line's count: zeros (-1 for a state)
    for (uint64_t t = count + tid; t < F; t += ALAC_PYIN_DECODE_THREADS) {
        if (out) out[t] = 0.0f, out[F + t] = 0.0f, out[2u * F + t] = 0.0f;
        if (states) states[t] = -1;
    }
    if (count == 0u) return;                                       // (the whole workgroup: no recursion)
    const float* ov = p.obs_voiced + (uint64_t)plane * F * n;
    const float* ou = p.obs_unvoiced + (uint64_t)plane * F;
    uint16_t* back = p.back + (uint64_t)plane * F * S;
    if (out && p.vp)
        for (uint64_t t = tid; t < count; t += ALAC_PYIN_DECODE_THREADS) out[2u * F + t] = p.vp[(uint64_t)plane * F + t];
    for (uint32_t i = tid; i <= band; i += ALAC_PYIN_DECODE_THREADS) lt_lds[i] = p.tab.lt[i];
    const float ls_stay = p.tab.ls[0], ls_switch = p.tab.ls[1], lstart = p.tab.lstart[0];
    {
        const float u0 = ou[0];
        for (uint32_t i = tid; i < n; i += ALAC_PYIN_DECODE_THREADS) {
            const float lz = p.tab.lz[i];
            const float dv = __fadd_rn(lstart, ov[i]), du = __fadd_rn(lstart, u0);
            lz_lds[i] = lz;
            delta_lds[i] = dv, delta_lds[n + i] = du;
            e_lds[0][i] = __fsub_rn(dv, lz), e_lds[0][n + i] = __fsub_rn(du, lz);
        }
    }
    __syncthreads();
    for (uint64_t t = 1u; t < count; t++) {
        const float* ev = e_lds[(t - 1u) & 1u];
        const float* eu = ev + n;
        float* next = e_lds[t & 1u];
        const float obs_u = ou[t];
        const float* obs_v = ov + t * n;
        uint16_t* from = back + t * S;
        for (uint32_t i = tid; i < n; i += ALAC_PYIN_DECODE_THREADS) {
            const uint32_t j0 = i > band ? i - band : 0u, j1 = i + band < n ? i + band : n - 1u;
            float mv = 0.0f, mu = 0.0f;
            uint32_t av = j0, au = j0;
            for (uint32_t j = j0; j <= j1; j++) {                  // ascending sources: the lowest wins a tie
                const float l = lt_lds[j < i ? i - j : j - i];
                const float cv = __fadd_rn(ev[j], l), cu = __fadd_rn(eu[j], l);
                if (j == j0 || cv > mv) mv = cv, av = j;
                if (j == j0 || cu > mu) mu = cu, au = j;
            }
            const float lz = lz_lds[i];
            // the voiced target: stay from the voiced half, switch from the unvoiced; a tie: the voiced source
            float a = __fadd_rn(mv, ls_stay), b = __fadd_rn(mu, ls_switch);
            bool take = b > a;
            const float dv = __fadd_rn(obs_v[i], take ? b : a);
            from[i] = (uint16_t)(take ? n + au : av);
            // the unvoiced target
            a = __fadd_rn(mv, ls_switch), b = __fadd_rn(mu, ls_stay);
            take = b > a;
            const float du = __fadd_rn(obs_u, take ? b : a);
            from[n + i] = (uint16_t)(take ? n + au : av);
            delta_lds[i] = dv, delta_lds[n + i] = du;
            next[i] = __fsub_rn(dv, lz), next[n + i] = __fsub_rn(du, lz);
        }
        __syncthreads();                                           // (next is read, and the other buffer written, behind it)
    }
    // the first arg-max of the last delta: a lane's states ascend, then lexicographic (larger value, lower state)
    float best = -__builtin_inff();
    uint32_t at = 0xFFFFFFFFu;
    for (uint32_t s = tid; s < S; s += ALAC_PYIN_DECODE_THREADS) {
        const float v = delta_lds[s];
        if (at == 0xFFFFFFFFu || v > best) best = v, at = s;
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const float ob = __shfl_xor(best, w, 64);
        const uint32_t oa = (uint32_t)__shfl_xor((int)at, w, 64);
        if (oa != 0xFFFFFFFFu && (at == 0xFFFFFFFFu || ob > best || (ob == best && oa < at))) best = ob, at = oa;
    }
    if ((tid & 63u) == 0u) best_lds[tid >> 6] = best, at_lds[tid >> 6] = at;
    __syncthreads();                                               // (and the backpointers of the last frame are visible)
    if (tid != 0u) return;
    for (uint32_t w = 1u; w < ALAC_PYIN_DECODE_THREADS / 64; w++) {
        const float ob = best_lds[w];
        const uint32_t oa = at_lds[w];
        if (oa != 0xFFFFFFFFu && (ob > best || (ob == best && oa < at))) best = ob, at = oa;
    }
    // the walk back, one dependent load a frame
    uint32_t s = at;
    for (uint64_t t = count; t-- > 0u;) {
        if (out) out[t] = p.tab.freq[s < n ? s : s - n], out[F + t] = s < n ? 1.0f : 0.0f;
        if (states) states[t] = (int32_t)s;
        if (t) s = back[t * S + s];
    }
}
