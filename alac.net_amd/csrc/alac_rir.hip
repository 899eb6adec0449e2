// alac_rir.hip -- image-source responses of shoebox rooms, one wave per (row, tile of 64 taps).  alac_rir.h states the scheme,
// alac.net_amd/rir.py every operation.  The geometry of an image -- coordinates, distance, delay and its split into k0 and f
// -- is float64, each operation rounded once (the root through __dsqrt_rn, the box's quotients through __ddiv_rn); everything
// per tap is float32 from explicit polynomials, no library sine, cosine or power.  The file is compiled with
// -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: no multiply is fused into an add, `/` on floats is the correctly
// rounded division.
#include "alac_rir.h"

#pragma clang fp contract(off)

namespace {

constexpr float PI_F = 3.1415927f;
constexpr double FOUR_PI = 4.0 * 3.14159265358979323846;
constexpr float S1 = -0.16666667f, S2 = 0.008333334f, S3 = -0.0001984127f, S4 = 2.7557319e-06f, S5 = -2.5052108e-08f, S6 = 1.6059044e-10f;
constexpr float C1 = -0.5f, C2 = 0.041666668f, C3 = -0.0013888889f, C4 = 2.4801588e-05f, C5 = -2.755732e-07f, C6 = 2.0876756e-09f;

__device__ inline float sin_poly(float x) {
    const float z = x * x;
    float q = S6;
    q = q * z + S5;
    q = q * z + S4;
    q = q * z + S3;
    q = q * z + S2;
    q = q * z + S1;
    return x + (x * z) * q;
}

__device__ inline float cos_poly(float x) {
    const float z = x * x;
    float q = C6;
    q = q * z + C5;
    q = q * z + C4;
    q = q * z + C3;
    q = q * z + C2;
    q = q * z + C1;
    return 1.0f + z * q;
}

// The recurrence of the powers: square and multiply from the lowest bit
__device__ inline float pow_rec(float b, uint32_t e) {
    float r = 1.0f;
    while (e) {
        if (e & 1u) r = r * b;
        b = b * b;
        e >>= 1;
    }
    return r;
}

__device__ inline uint32_t iabs(int v) { return (uint32_t)(v < 0 ? -v : v); }

// The coordinate of image (n, p) on one axis
__device__ inline double coord(double s, double L, double r, int n, int p) { return ((p ? -s : s) + (double)(2 * n) * L) - r; }

// min and max over p of the squared coordinate
__device__ inline void span2(double s, double L, double r, int n, double& lo2, double& hi2) {
    const double a = fabs(coord(s, L, r, n, 0)), b = fabs(coord(s, L, r, n, 1));
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    lo2 = lo * lo;
    hi2 = hi * hi;
}

struct lists {
    int nx[ALAC_RIR_LIST], ny[ALAC_RIR_LIST], zp[ALAC_RIR_LIST], k0[ALAC_RIR_LIST];
    float ff[ALAC_RIR_LIST], fpd[ALAC_RIR_LIST], sp[ALAC_RIR_LIST], cphi[ALAC_RIR_LIST], sphi[ALAC_RIR_LIST], amp[ALAC_RIR_LIST];
    float cw[64], sw[64];
};

}  // namespace

__global__ __launch_bounds__(ALAC_RIR_THREADS) void alac_rir_shoebox_kernel(alac_rir_params p) {
    __shared__ lists S;
    const uint32_t lane = threadIdx.x;
    const uint32_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int K = (int)p.frames, H = (int)(p.taps / 2u);
    const int k_lo = (int)(tile * ALAC_RIR_TILE), k_hi = k_lo + (int)ALAC_RIR_TILE < K ? k_lo + (int)ALAC_RIR_TILE : K;
    const int k = k_lo + (int)lane;
    float* const out = p.out + (uint64_t)row * p.out_stride;
    const double* const G = p.geometry + (uint64_t)row * 9u;
    double L[3], s[3], r[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        L[a] = G[a];
        s[a] = G[3 + a];
        r[a] = G[6 + a];
        ok = ok && isfinite(L[a]) && isfinite(s[a]) && isfinite(r[a]) && L[a] > 0.0 && s[a] >= 0.0 && s[a] <= L[a] && r[a] >= 0.0 && r[a] <= L[a];
    }
    // the candidate box, and with it the refusal
    int N[3] = {0, 0, 0};
    if (ok) {
        const double dmax = __ddiv_rn((double)(K + H + H + 1), p.scale);
        double count = 8.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double q = __ddiv_rn(dmax, L[a] + L[a]);
            if (!(q < ALAC_RIR_MAX_QUOTIENT)) {
                ok = false;
                break;
            }
            int n = (int)q + 2;
            if (p.max_order >= 0 && n > (p.max_order >> 1) + (p.max_order & 1)) n = (p.max_order >> 1) + (p.max_order & 1);
            N[a] = n;
            count *= (double)(2 * n + 1);
        }
        ok = ok && !(count > ALAC_RIR_LIMIT);
    }
    if (tile == 0u && lane == 0u) p.lengths[row] = ok ? K : 0;
    if (!ok) {
        if (k < K) out[k] = 0.0f;
        return;
    }
    S.cw[lane] = p.cw[lane];
    S.sw[lane] = p.sw[lane];
    float b[6];
#pragma unroll
    for (int a = 0; a < 6; a++) b[a] = p.beta[(uint64_t)row * 6u + a];

    // the tile's shell of distances, half a tap and more of slack on either side
    const double d_lo = k_lo - H - 1 > 0 ? __ddiv_rn((double)(k_lo - H - 1), p.scale) : 0.0;
    const double d_hi = __ddiv_rn((double)(k_hi + H), p.scale);
    const double d_lo2 = d_lo * d_lo, d_hi2 = d_hi * d_hi;
    const double two_lz = L[2] + L[2];
    const unsigned long long below = (1ull << lane) - 1ull;
    float acc = 0.0f;
    uint32_t listed = 0;

    // The list's images into every lane's tap, in the list's order
    auto flush = [&](uint32_t n) {
        __syncthreads();
        for (uint32_t i = lane; i < n; i += 64u) {
            const int nx = S.nx[i], ny = S.ny[i], zp = S.zp[i];
            const int nz = zp >> 3, px = (zp >> 2) & 1, py = (zp >> 1) & 1, pz = zp & 1;
            const float g = ((pow_rec(b[0], iabs(nx - px)) * pow_rec(b[1], iabs(nx))) * (pow_rec(b[2], iabs(ny - py)) * pow_rec(b[3], iabs(ny)))) *
                            (pow_rec(b[4], iabs(nz - pz)) * pow_rec(b[5], iabs(nz)));
            const float ff = S.ff[i];
            const float phi = p.tw * ff;
            S.amp[i] = g / S.fpd[i];
            S.sp[i] = sin_poly(PI_F * ff);
            S.cphi[i] = cos_poly(phi);
            S.sphi[i] = sin_poly(phi);
        }
        __syncthreads();
        for (uint32_t i = 0; i < n; i++) {
            const int m = k - S.k0[i];
            if (m >= -H && m <= H) {
                const uint32_t am = iabs(m);
                const float cwm = S.cw[am], swm = m < 0 ? -S.sw[am] : S.sw[am];
                const float ff = S.ff[i], sp = S.sp[i];
                const float u = cwm * S.cphi[i], v = swm * S.sphi[i];
                const float c = u + v;
                const float w = 0.5f + 0.5f * c;
                const float tt = (float)m - ff;
                const float num = (m & 1) ? sp : -sp;
                const float den = PI_F * tt;
                const float sinc = tt == 0.0f ? 1.0f : num / den;
                const float ws = w * sinc;
                acc = acc + S.amp[i] * ws;
            }
        }
        __syncthreads();
    };

    for (int nx = -N[0]; nx <= N[0]; nx++) {
        double x_lo2, x_hi2;
        span2(s[0], L[0], r[0], nx, x_lo2, x_hi2);
        if (x_lo2 > d_hi2) continue;
        for (int ny_base = -N[1]; ny_base <= N[1]; ny_base += 64) {
            // a lane solves a pair (nx, ny): nz in -top .. -(hole + 1) and max(hole + 1, 1) .. top, or none (top < 0)
            const int my_ny = ny_base + (int)lane;
            int top = -1, hole = -1;
            if (my_ny <= N[1]) {
                double y_lo2, y_hi2;
                span2(s[1], L[1], r[1], my_ny, y_lo2, y_hi2);
                const double zz = d_hi2 - (x_lo2 + y_lo2);
                if (zz >= 0.0) {
                    const double qt = __ddiv_rn(__dsqrt_rn(zz), two_lz);
                    top = qt < (double)N[2] ? (int)qt + 2 : N[2];
                    if (top > N[2]) top = N[2];
                    const double inner = d_lo2 - (x_hi2 + y_hi2);
                    if (inner > 0.0) {
                        const double qh = __ddiv_rn(__dsqrt_rn(inner), two_lz);
                        hole = qh < (double)N[2] + 4.0 ? (int)qh - 2 : N[2] + 2;
                        if (hole < -1) hole = -1;
                    }
                }
            }
            const int pairs = N[1] - ny_base + 1 < 64 ? N[1] - ny_base + 1 : 64;
            for (int i = 0; i < pairs; i++) {
                const int t = __builtin_amdgcn_readfirstlane(__shfl(top, i, 64));
                if (t < 0) continue;
                const int h = __builtin_amdgcn_readfirstlane(__shfl(hole, i, 64));
                const int ny = ny_base + i;
                const int first_pos = h + 1 > 1 ? h + 1 : 1;
                const int c_neg = t - h > 0 ? t - h : 0, c_pos = t - first_pos + 1 > 0 ? t - first_pos + 1 : 0;
                const int total = 8 * (c_neg + c_pos);
                for (int j0 = 0; j0 < total; j0 += 64) {
                    const int j = j0 + (int)lane;
                    bool reach = false;
                    int nz = 0, pi = 0, k0 = 0;
                    float ff = 0.0f, fpd = 0.0f;
                    if (j < total) {
                        const int q = j >> 3;
                        pi = j & 7;
                        nz = q < c_neg ? -t + q : first_pos + (q - c_neg);
                        const int px = pi >> 2, py = (pi >> 1) & 1, pz = pi & 1;
                        const double xx = coord(s[0], L[0], r[0], nx, px), xy = coord(s[1], L[1], r[1], ny, py), xz = coord(s[2], L[2], r[2], nz, pz);
                        const double d = __dsqrt_rn((xx * xx + xy * xy) + xz * xz);
                        const double tau = d * p.scale;
                        const double kf = floor(tau + 0.5);
                        if (kf - (double)H <= (double)(k_hi - 1)) {       // (false for a tau that is not finite, too)
                            k0 = (int)kf;
                            ff = (float)(tau - kf);
                            fpd = (float)(FOUR_PI * d);
                            reach = k0 + H >= k_lo;
                            if (p.max_order >= 0 && (int)(iabs(2 * nx - px) + iabs(2 * ny - py) + iabs(2 * nz - pz)) > p.max_order) reach = false;
                        }
                    }
                    const unsigned long long mask = __ballot(reach);
                    if (reach) {
                        const uint32_t at = listed + (uint32_t)__popcll(mask & below);
                        S.nx[at] = nx;
                        S.ny[at] = ny;
                        S.zp[at] = nz * 8 + pi;
                        S.k0[at] = k0;
                        S.ff[at] = ff;
                        S.fpd[at] = fpd;
                    }
                    listed = (uint32_t)__builtin_amdgcn_readfirstlane((int)(listed + (uint32_t)__popcll(mask)));
                    if (listed >= 64u) {
                        flush(listed);
                        listed = 0;
                    }
                }
            }
        }
    }
    if (listed) flush(listed);
    if (k < K) out[k] = acc;
}
