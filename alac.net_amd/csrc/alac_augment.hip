// alac_augment.hip -- SpecAugment behind the features: a time warp, frequency masks and time masks per crop, one launch.
// include/alacgpu.h and alac.net_amd/augment.py state the arithmetic, alac_augment.h the mappings and the thresholds.  The
// interpolation of the warp is three IEEE float32 operations rounded once each behind one correctly rounded division: this
// file is compiled with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt, and the operations go through
// __fsub_rn / __fmul_rn / __fadd_rn.  src and out may be the same array: a line that is warped is in LDS as a whole before
// any of it is written, and a line that is not is written where it is masked and nowhere else, without being read.
#include "alac_augment.h"

#pragma clang fp contract(off)

namespace {

// What the G threads of a line know of it; all of it is the same in every one of them
struct aug_line {
    const float* x;
    float* y;
    const int2* tab;              // LDS: the row's time masks as (first, behind the last), cut to 0 .. tau
    const float* stage;           // LDS: the frames 0 .. tau of a warped line
    uint32_t n_time;
    uint64_t n, tau;
    uint32_t c, c1;               // the warp (c, c'), when `warped`
    bool warped, fline, inplace;
    float fill;

    __device__ bool masked(uint64_t t) const {
        if (t >= tau) return false;
        if (fline) return true;
        for (uint32_t k = 0; k < n_time; k++) {
            const int2 m = tab[k];
            if (t >= (uint64_t)m.x && t < (uint64_t)m.y) return true;      // (an empty span is x = y = 0)
        }
        return false;
    }

    // Frame t < tau of the warped line: x[i] + f * (x[i + 1] - x[i]) at the source position i + r / den.  t, c, c' and tau
    // are at most ALAC_AUG_LDS_MAX, so the products are below 2^28 and r and den are exact in float32.
    __device__ float warp_at(uint32_t t) const {
        uint32_t num, den, i0;
        if (t <= c1) {
            num = t * c;
            den = c1;
            i0 = 0u;
        } else {
            num = (t - c1) * ((uint32_t)tau - 1u - c);
            den = (uint32_t)tau - 1u - c1;
            i0 = c;
        }
        const uint32_t q = num / den, r = num - q * den, i = i0 + q;
        const float a = stage[i];
        if (r == 0u) return a;
        const float f = (float)r / (float)den;
        return __fadd_rn(a, __fmul_rn(f, __fsub_rn(stage[i + 1u], a)));
    }

    // Frame t as it has to be written; false: it stays as it is (in place, neither masked nor warped)
    __device__ bool value(uint64_t t, float& v) const {
        if (masked(t)) v = fill;
        else if (warped && t < tau) v = warp_at((uint32_t)t);
        else if (!inplace) v = x[t];
        else return false;
        return true;
    }
};

// The G threads of a line (g: this thread among them), behind the barrier that follows the staging
template <uint32_t G>
__device__ inline void write_line(const aug_line& L, uint32_t g) {
    // 128-bit accesses where x and y are 16 bytes aligned at the same frames: the frames in front of the first such frame
    // (head) and behind the last whole four are written one by one
    const uintptr_t ax = (uintptr_t)L.x, ay = (uintptr_t)L.y;
    const bool vec = ((ax ^ ay) & 15u) == 0u;
    uint64_t head = vec ? ((16u - (ay & 15u)) >> 2) & 3u : L.n;
    if (head > L.n) head = L.n;
    const uint64_t quads = (L.n - head) >> 2;
    for (uint64_t t = g; t < head; t += G) {
        float v;
        if (L.value(t, v)) L.y[t] = v;
    }
    for (uint64_t t = head + 4u * quads + g; t < L.n; t += G) {
        float v;
        if (L.value(t, v)) L.y[t] = v;
    }
    for (uint64_t q = g; q < quads; q += G) {
        const uint64_t t0 = head + 4u * q;
        const bool m0 = L.masked(t0), m1 = L.masked(t0 + 1u), m2 = L.masked(t0 + 2u), m3 = L.masked(t0 + 3u);
        float4* const dst = (float4*)(L.y + t0);
        if (m0 && m1 && m2 && m3) {                               // a span: stored, never loaded
            *dst = make_float4(L.fill, L.fill, L.fill, L.fill);
        } else if (L.warped && t0 + 4u <= L.tau) {
            const uint32_t t = (uint32_t)t0;
            *dst = make_float4(m0 ? L.fill : L.warp_at(t), m1 ? L.fill : L.warp_at(t + 1u), m2 ? L.fill : L.warp_at(t + 2u),
                               m3 ? L.fill : L.warp_at(t + 3u));
        } else if (!L.inplace && !(L.warped && t0 < L.tau)) {     // a copy but for the masked frames
            const float4 a = *(const float4*)(L.x + t0);
            *dst = make_float4(m0 ? L.fill : a.x, m1 ? L.fill : a.y, m2 ? L.fill : a.z, m3 ? L.fill : a.w);
        } else {                                                  // in place, or the four frames around tau of a warped line
            float v;
            if (L.value(t0, v)) L.y[t0] = v;
            if (L.value(t0 + 1u, v)) L.y[t0 + 1u] = v;
            if (L.value(t0 + 2u, v)) L.y[t0 + 2u] = v;
            if (L.value(t0 + 3u, v)) L.y[t0 + 3u] = v;
        }
    }
}

// LINES lines to a workgroup, G = ALAC_AUG_THREADS / LINES threads to a line.  Dynamic LDS: per line the time-mask table
// (n_time int2), then, behind the tables of all lines, `stage` floats per line.
template <uint32_t LINES>
__device__ inline void augment(const alac_augment_params& p) {
    constexpr uint32_t G = ALAC_AUG_THREADS / LINES;
    extern __shared__ int2 aug_lds[];
    const uint32_t slot = threadIdx.x / G, g = threadIdx.x % G;
    const uint64_t l = (uint64_t)blockIdx.x * LINES + slot;
    int2* const tab = aug_lds + (size_t)slot * p.n_time;
    float* const stage = (float*)(aug_lds + (size_t)LINES * p.n_time) + (size_t)slot * p.stage;
    aug_line L = {};
    const bool live = l < p.lines;                                // (no thread leaves in front of the barrier)
    if (live) {
        const uint64_t row = l / p.lines_per_row;
        const uint32_t bin = (uint32_t)(l % p.n_mels);
        L.x = p.src + l * p.line_stride;
        L.y = p.out + l * p.line_stride;
        L.tab = tab;
        L.stage = stage;
        L.n_time = p.n_time;
        L.n = p.line_len;
        L.tau = p.line_len;
        if (p.valid) {
            const int64_t a = p.valid[row];
            L.tau = a <= 0 ? 0u : ((uint64_t)a < p.line_len ? (uint64_t)a : p.line_len);
        }
        L.inplace = p.src == p.out;
        L.fill = p.fill;
        if (p.warp && p.stage && L.tau >= 3u) {
            const int64_t c = p.warp[2u * row], c1 = p.warp[2u * row + 1u], last = (int64_t)L.tau - 2;
            L.warped = c != c1 && c >= 1 && c1 >= 1 && c <= last && c1 <= last;
            L.c = (uint32_t)c;
            L.c1 = (uint32_t)c1;
        }
        for (uint32_t k = 0; k < p.n_freq; k++) {
            const int32_t* const m = p.freq + 2u * (row * p.n_freq + k);
            const int64_t lo = m[0], hi = lo + m[1];
            L.fline |= m[1] > 0 && (int64_t)bin >= lo && (int64_t)bin < hi;
        }
        for (uint32_t k = g; k < p.n_time; k += G) {
            const int32_t* const m = p.time + 2u * (row * p.n_time + k);
            const int64_t tau = (int64_t)L.tau;
            int64_t lo = m[0], hi = lo + m[1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > tau ? tau : hi;
            tab[k] = m[1] > 0 && lo < hi ? make_int2((int)lo, (int)hi) : make_int2(0, 0);
        }
        if (L.warped && !L.fline) {                               // the valid frames, all of them, before any is written
            const uint64_t first = ((16u - ((uintptr_t)L.x & 15u)) >> 2) & 3u, head = first < L.tau ? first : L.tau;
            const uint64_t quads = (L.tau - head) >> 2;
            for (uint64_t t = g; t < head; t += G) stage[t] = L.x[t];
            for (uint64_t t = head + 4u * quads + g; t < L.tau; t += G) stage[t] = L.x[t];
            for (uint64_t q = g; q < quads; q += G) {
                const uint64_t t0 = head + 4u * q;
                const float4 a = *(const float4*)(L.x + t0);
                stage[t0] = a.x;
                stage[t0 + 1u] = a.y;
                stage[t0 + 2u] = a.z;
                stage[t0 + 3u] = a.w;
            }
        }
    }
    __syncthreads();
    if (live) write_line<G>(L, g);
}

}  // namespace

__global__ __launch_bounds__(ALAC_AUG_THREADS) void alac_specaugment_wave_kernel(alac_augment_params p) { augment<ALAC_AUG_WAVE_LINES>(p); }

__global__ __launch_bounds__(ALAC_AUG_THREADS) void alac_specaugment_line_kernel(alac_augment_params p) { augment<1u>(p); }
