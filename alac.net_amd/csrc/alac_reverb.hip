// alac_reverb.hip -- room reverberation into the crops, between the waveform and the noise mix: a uniformly partitioned
// overlap-save convolution of every crop with its impulse response.  An analyse launch (the spectra of every block of the
// signal and of every partition of the impulse response, and per row the direct path d, the gain g and whether the row is
// left alone) and a synthesise launch (per block of the output the sum over the partitions of X[m - p] . H[p], one inverse
// transform, the shift by d, the product with g), no atomics.  include/alacgpu.h states the arithmetic, alac_reverb.h the
// blocks, the transform, the layout of the spectra and the order of the sums.  Every operation is one IEEE float32 operation,
// rounded once: this file is compiled with -ffp-contract=off and the products and sums go through __fmul_rn / __fadd_rn /
// __fsub_rn; the division is `/` and the root sqrtf, which -fhip-fp32-correctly-rounded-divide-sqrt makes the correctly
// rounded ones.  src and out may be the same array: the synthesise launch reads the spectra, not the signal.
#include "alac_reverb.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t N = ALAC_REVERB_N, HOP = ALAC_REVERB_HOP, THREADS = ALAC_REVERB_THREADS;

// min(max(valid[row], 0), frames), frames without `valid`
__device__ inline uint64_t valid_of(const int64_t* valid, uint32_t row, uint64_t frames) {
    if (!valid) return frames;
    const int64_t a = valid[row];
    return a <= 0 ? 0u : ((uint64_t)a < frames ? (uint64_t)a : frames);
}

__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)); }
__device__ inline float2 cmul(float2 a, float2 b) {
    return make_float2(__fsub_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fadd_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x)));
}
__device__ inline float2 conj(float2 a) { return make_float2(a.x, -a.y); }

// The forward transform of z[N] in LDS, in place, natural order in, base-4 digit-reversed order out (alac_reverb.h).  A
// butterfly reads and writes its own four elements; a barrier stands in front of every stage and behind the last.
__device__ inline void forward(float2* z, const float2* tw) {
    for (uint32_t L = N / 4u; L >= 1u; L >>= 2) {
        const uint32_t step = N / (4u * L);
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < N / 4u; q += THREADS) {
            const uint32_t j = q & (L - 1u), i0 = ((q - j) << 2) + j;
            const float2 a = z[i0], b = z[i0 + L], c = z[i0 + 2u * L], d = z[i0 + 3u * L];
            const float2 t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), bd = csub(b, d);
            const float2 t3 = make_float2(bd.y, -bd.x);                       // -i (b - d)
            z[i0] = cadd(t0, t2);
            z[i0 + L] = cmul(cadd(t1, t3), tw[j * step]);
            z[i0 + 2u * L] = cmul(csub(t0, t2), tw[2u * j * step]);
            z[i0 + 3u * L] = cmul(csub(t1, t3), tw[3u * j * step]);
        }
    }
    __syncthreads();
}

// The inverse transform, not divided by N: digit-reversed order in, natural order out; the forward stages' conjugate
// transposes in the opposite order
__device__ inline void inverse(float2* z, const float2* tw) {
    for (uint32_t L = 1u; L <= N / 4u; L <<= 2) {
        const uint32_t step = N / (4u * L);
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < N / 4u; q += THREADS) {
            const uint32_t j = q & (L - 1u), i0 = ((q - j) << 2) + j;
            const float2 z0 = z[i0], z1 = cmul(z[i0 + L], conj(tw[j * step])), z2 = cmul(z[i0 + 2u * L], conj(tw[2u * j * step])),
                         z3 = cmul(z[i0 + 3u * L], conj(tw[3u * j * step]));
            const float2 u0 = cadd(z0, z2), u1 = csub(z0, z2), u2 = cadd(z1, z3), dz = csub(z1, z3);
            const float2 u3 = make_float2(-dz.y, dz.x);                       // i (z1 - z3)
            z[i0] = cadd(u0, u2);
            z[i0 + L] = cadd(u1, u3);
            z[i0 + 2u * L] = csub(u0, u2);
            z[i0 + 3u * L] = csub(u1, u3);
        }
    }
    __syncthreads();
}

// d, g and whether the row is left alone, in alac_reverb.h's order; lds: 4 * THREADS floats
__device__ inline void verdict(const alac_reverb_params& p, uint32_t row, uint64_t v, uint64_t vh, float* lds) {
    float* const qs = lds;
    float* const bs = lds + THREADS;
    uint64_t* const at = reinterpret_cast<uint64_t*>(lds + 2u * THREADS);
    const uint32_t t = threadIdx.x;
    float s = 0.0f, best = -1.0f;
    uint64_t first = UINT64_MAX;
    if (v != 0u && vh != 0u) {
        for (uint32_t c = 0; c < p.rir_channels; c++) {
            const float* h = p.rir + ((uint64_t)row * p.rir_channels + c) * p.rir_stride;
            for (uint64_t k = t; k < vh; k += THREADS) {
                const float a = h[k];
                s = __fadd_rn(s, __fmul_rn(a, a));
                if (c == 0u && fabsf(a) > best) best = fabsf(a), first = k;
            }
        }
    }
    qs[t] = s, bs[t] = best, at[t] = first;
    for (uint32_t h = THREADS / 2u; h >= 1u; h >>= 1) {
        __syncthreads();
        if (t < h) {
            qs[t] = __fadd_rn(qs[t], qs[t + h]);
            if (bs[t + h] > bs[t] || (bs[t + h] == bs[t] && at[t + h] < at[t])) bs[t] = bs[t + h], at[t] = at[t + h];
        }
    }
    if (t == 0u) {
        const float e = qs[0] / (float)p.rir_channels;
        alac_reverb_row r;
        r.live = v != 0u && vh != 0u && e > 0.0f && e < __builtin_inff() ? 1u : 0u;      // (a NaN compares false)
        r.g = r.live ? 1.0f / sqrtf(e) : 0.0f;
        r.d = at[0] < vh ? at[0] : 0u;
        p.verdict[row] = r;
    }
}

}  // namespace

// Unit blockIdx.x % units of row blockIdx.x / units: the spectrum of a block of a signal plane, of a partition of an impulse
// response plane, or (the last unit) the row's verdict.  A row with v == 0 or vh == 0 reads neither array.
__global__ __launch_bounds__(ALAC_REVERB_THREADS) void alac_reverb_analyse_kernel(alac_reverb_params p) {
    __shared__ __align__(16) float2 z[N];
    const uint32_t row = blockIdx.x / p.units, unit = blockIdx.x % p.units;
    const uint64_t v = valid_of(p.valid, row, p.frames), vh = valid_of(p.rir_valid, row, p.rir_frames);
    if (unit == p.units - 1u) {
        verdict(p, row, v, vh, reinterpret_cast<float*>(z));
        return;
    }
    if (v == 0u || vh == 0u) return;                      // (the row's: every thread returns or none)
    const uint32_t nx = p.channels * p.x_blocks;
    const float* plane;
    int64_t first;                                        // the block holds plane[first + t], t < span, where 0 <= first + t < end
    uint64_t end;
    uint32_t span;
    if (unit < nx) {
        const uint32_t c = unit / p.x_blocks, j = unit % p.x_blocks;
        first = ((int64_t)j - 1) * (int64_t)HOP;
        if (first >= (int64_t)v) return;                  // no frame below v
        plane = p.src + ((uint64_t)row * p.channels + c) * p.stride;
        end = v;
        span = N;
    } else {
        const uint32_t c = (unit - nx) / p.rir_parts, part = (unit - nx) % p.rir_parts;
        first = (int64_t)part * (int64_t)HOP;
        if (first >= (int64_t)vh) return;                 // no frame below vh
        plane = p.rir + ((uint64_t)row * p.rir_channels + c) * p.rir_stride;
        end = vh;
        span = HOP;
    }
    for (uint32_t t = threadIdx.x; t < N; t += THREADS) {
        const int64_t i = first + (int64_t)t;
        z[t] = make_float2(t < span && i >= 0 && (uint64_t)i < end ? plane[i] : 0.0f, 0.0f);
    }
    forward(z, p.twiddles);
    float4* const dst = reinterpret_cast<float4*>(p.spectra + ((uint64_t)row * (p.units - 1u) + unit) * N);
    for (uint32_t t = threadIdx.x; t < N / 2u; t += THREADS) dst[t] = reinterpret_cast<const float4*>(z)[t];
}

// Block blockIdx.x % out_blocks of the convolution of plane blockIdx.x / out_blocks: w[n] for n = m H .. (m + 1) H, of which
// y[n - d] = g w[n] is stored where 0 <= n - d < v.  Out of place the workgroup also copies the frames m H .. (m + 1) H of x
// that stay (those at or behind v; all of a row that is left alone).
__global__ __launch_bounds__(ALAC_REVERB_THREADS) void alac_reverb_synth_kernel(alac_reverb_params p) {
    __shared__ __align__(16) float2 z[N];
    constexpr uint32_t PAIRS = N / 2u / THREADS;          // float4 = two bins; a thread's share of a spectrum
    const uint32_t m = blockIdx.x % p.out_blocks;
    const uint64_t plane = blockIdx.x / p.out_blocks;
    const uint32_t row = (uint32_t)(plane / p.channels), c = (uint32_t)(plane % p.channels);
    const uint64_t v = valid_of(p.valid, row, p.frames), vh = valid_of(p.rir_valid, row, p.rir_frames);
    const alac_reverb_row r = p.verdict[row];
    const float* x = p.src + plane * p.stride;
    float* y = p.out + plane * p.stride;
    const uint64_t n0 = (uint64_t)m * HOP;
    if (p.out != p.src) {
        const uint64_t from = r.live ? v : 0u, end = n0 + HOP < p.frames ? n0 + HOP : p.frames;
        for (uint64_t i = n0 + threadIdx.x; i < end; i += THREADS)
            if (i >= from) y[i] = x[i];
    }
    if (!r.live || n0 + HOP <= r.d || n0 >= r.d + v) return;         // (the workgroup's: every thread returns or none)
    const uint64_t last_x = (v + HOP - 1u) / HOP, parts = (vh + HOP - 1u) / HOP;       // the last block of x, the partitions of h
    const uint64_t p_lo = m > last_x ? m - last_x : 0u, p_hi = m < parts - 1u ? m : parts - 1u;
    const uint64_t base = (uint64_t)row * (p.units - 1u);
    const float4* const X = reinterpret_cast<const float4*>(p.spectra + (base + (uint64_t)c * p.x_blocks) * N);
    const float4* const Hs = reinterpret_cast<const float4*>(
        p.spectra + (base + (uint64_t)p.channels * p.x_blocks + (uint64_t)(p.rir_channels == 1u ? 0u : c) * p.rir_parts) * N);
    float4 acc[PAIRS];
#pragma unroll
    for (uint32_t k = 0; k < PAIRS; k++) acc[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint64_t part = p_lo; part <= p_hi; part++) {
        const float4* const xb = X + ((uint64_t)m - part) * (N / 2u);
        const float4* const hb = Hs + part * (N / 2u);
#pragma unroll
        for (uint32_t k = 0; k < PAIRS; k++) {
            const float4 a = xb[threadIdx.x + k * THREADS], b = hb[threadIdx.x + k * THREADS];
            const float2 lo = cmul(make_float2(a.x, a.y), make_float2(b.x, b.y)), hi = cmul(make_float2(a.z, a.w), make_float2(b.z, b.w));
            acc[k] = make_float4(__fadd_rn(acc[k].x, lo.x), __fadd_rn(acc[k].y, lo.y), __fadd_rn(acc[k].z, hi.x), __fadd_rn(acc[k].w, hi.y));
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < PAIRS; k++) reinterpret_cast<float4*>(z)[threadIdx.x + k * THREADS] = acc[k];
    inverse(z, p.twiddles);
    for (uint32_t t = threadIdx.x; t < HOP; t += THREADS) {
        const uint64_t n = n0 + t;
        if (n >= r.d && n - r.d < v) y[n - r.d] = __fmul_rn(r.g, __fmul_rn(z[HOP + t].x, 1.0f / (float)N));
    }
}
