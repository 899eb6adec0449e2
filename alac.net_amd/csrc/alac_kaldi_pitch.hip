// alac_kaldi_pitch.hip -- Kaldi's pitch features behind the crops (Ghahremani et al. 2014), three launches: the downsampled rows
// with the partial sums of their mean square, the NCCF of every frame on the lag grid, and the dense Viterbi decode along every
// plane with the post-processing as its epilogue.  alac_kaldi_pitch.h states the parameters and the layouts,
// alac.net_amd/kaldi_pitch.py every operation in order.  Float32, one IEEE operation at a time (the row sums of the ballast
// float64): this file is compiled with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt, the multiply-adds are the
// __fmaf_rn written, `/` and sqrtf the correctly rounded ones, the logarithm and the exponential alac_pcen.h's explicit
// polynomials.  Every tie of the decode goes to the lowest source state: a candidate replaces the best so far only when it is
// strictly smaller, and candidates come in ascending order.  Plain vector stores only, no atomics.
#include "alac_kaldi_pitch.h"
#include "alac_pcen.h"

#pragma clang fp contract(off)

namespace {

constexpr float KP_LN2 = 0.693147180559945f, KP_LOG2E = 1.442695040888963f;

__device__ inline void kp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline uint64_t kp_valid(const int64_t* valid, uint32_t row, uint64_t most) {
    if (!valid) return most;
    const int64_t a = valid[row];
    return a <= 0 ? 0u : ((uint64_t)a < most ? (uint64_t)a : most);
}

// The tree of halves over the 64 lanes; every lane returns lane 0's sum
__device__ inline float kp_lane_tree(float part) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) part = __fadd_rn(part, __shfl_xor(part, w, 64));
    return __shfl(part, 0, 64);
}

__device__ inline float kp_exp(float x) { return alac_pcen_exp2(__fmul_rn(x, KP_LOG2E)); }

__device__ inline float kp_local(float n, float sl) { return __fadd_rn(__fsub_rn(1.0f, n), __fmul_rn(sl, n)); }

}  // namespace

__global__ __launch_bounds__(ALAC_KPITCH_THREADS) void alac_kpitch_down_kernel(alac_kpitch_down_params p) {
    __shared__ float w_lds[ALAC_KPITCH_MAX_DOWN];
    __shared__ double s_lds[ALAC_KPITCH_THREADS], q_lds[ALAC_KPITCH_THREADS];
    const uint32_t tid = threadIdx.x, chunk = blockIdx.x % p.chunks;
    const uint64_t plane = blockIdx.x / p.chunks;
    const uint32_t row = (uint32_t)(plane / p.channels);
    const uint64_t v = kp_valid(p.valid, row, p.frames), N = alac_kpitch_samples(p.fr, v);
    const uint32_t n_w = p.phases * p.down_taps;                   // (at most ALAC_KPITCH_MAX_DOWN: the host's check)
    for (uint32_t i = tid; i < n_w; i += ALAC_KPITCH_THREADS) w_lds[i] = p.tab.down[i];
    __syncthreads();
    const float* src = p.src + plane * p.stride;
    double s = 0.0, q = 0.0;
    for (uint32_t j = 0; j < ALAC_KPITCH_CHUNK / ALAC_KPITCH_THREADS; j++) {
        const uint64_t n = (uint64_t)chunk * ALAC_KPITCH_CHUNK + j * ALAC_KPITCH_THREADS + tid;
        float acc = 0.0f;
        if (n < N) {
            const uint64_t u = n / p.phases;
            const uint32_t ph = (uint32_t)(n % p.phases);
            const int64_t base = (int64_t)(u * p.in_per_unit) + (int64_t)p.tab.down_first[ph];
            const float* w = w_lds + (size_t)ph * p.down_taps;
            for (uint32_t k = 0; k < p.down_taps; k++) {
                const int64_t i = base + (int64_t)k;
                const float x = (i >= 0 && (uint64_t)i < v) ? src[i] : 0.0f;
                acc = __fmaf_rn(w[k], x, acc);
            }
            p.down[plane * p.n_max + n] = acc;                     // (n < N <= n_max)
        }
        const double d = (double)acc;
        s = s + d;
        q = q + d * d;
    }
    s_lds[tid] = s, q_lds[tid] = q;
    __syncthreads();
    for (uint32_t h = ALAC_KPITCH_THREADS / 2; h >= 1u; h >>= 1) {
        if (tid < h) s_lds[tid] = s_lds[tid] + s_lds[tid + h], q_lds[tid] = q_lds[tid] + q_lds[tid + h];
        __syncthreads();
    }
    if (tid == 0u) {
        double* o = p.sums + (plane * p.chunks + chunk) * 2u;
        o[0] = s_lds[0], o[1] = q_lds[0];
    }
}

__global__ __launch_bounds__(ALAC_KPITCH_THREADS) void alac_kpitch_nccf_kernel(alac_kpitch_nccf_params p) {
    extern __shared__ __align__(16) float kp_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t plane = blockIdx.x / p.groups;
    const uint64_t t = (uint64_t)(blockIdx.x % p.groups) * (ALAC_KPITCH_THREADS / 64) + wave;
    if (t >= p.out_frames) return;                                 // (a whole wave; the kernel has no workgroup barrier)
    const uint32_t row = (uint32_t)(plane / p.channels);
    const uint32_t W = p.fr.window, nl = p.last_lag - p.first_lag + 1u, span = W + p.last_lag, S = p.n_states;
    const uint64_t v = kp_valid(p.valid, row, p.frames), N = alac_kpitch_samples(p.fr, v);
    uint64_t count = alac_kpitch_frames(p.fr, v);
    if (count > p.out_frames) count = p.out_frames;
    float* o0 = p.nccf + ((plane * 2u) * p.out_frames + t) * S;
    float* o1 = p.nccf + ((plane * 2u + 1u) * p.out_frames + t) * S;
    if (t >= count) {                                              // at and behind the row's count: zeros
        for (uint32_t s = lane; s < S; s += 64u) o0[s] = 0.0f, o1[s] = 0.0f;
        return;
    }
    // the ballast from the row's partial sums, the chunks in ascending order (every lane the same)
    double rs = 0.0, rq = 0.0;
    {
        const uint64_t chunks = (N + ALAC_KPITCH_CHUNK - 1u) / ALAC_KPITCH_CHUNK;
        const double* sums = p.sums + plane * p.chunks * 2u;
        for (uint64_t c = 0; c < chunks; c++) rs = rs + sums[2u * c], rq = rq + sums[2u * c + 1u];
    }
    const double mean = rs / (double)N;
    const double b = (rq / (double)N - mean * mean) * (double)W;
    const float ballast = (float)(b * b * (double)p.tab.head[2]);
    float* a = kp_lds + (size_t)wave * (span + 2u * nl);
    float* nc = a + span;
    const float* d = p.down + plane * p.n_max;
    const float pre = p.tab.head[1];
    for (uint32_t i = lane; i < span; i += 64u) {
        const uint64_t g = t * p.fr.shift + i;
        float x = g < N ? d[g] : 0.0f;
        if (pre != 0.0f) {
            const float prev = i == 0u ? x : (g - 1u < N ? d[g - 1u] : 0.0f);
            x = __fsub_rn(x, __fmul_rn(pre, prev));
        }
        a[i] = x;
    }
    kp_wave_sync();
    float part = 0.0f;
    for (uint32_t i = lane; i < W; i += 64u) part = __fadd_rn(part, a[i]);
    const float m = kp_lane_tree(part) / (float)W;
    kp_wave_sync();
    for (uint32_t i = lane; i < span; i += 64u) a[i] = __fsub_rn(a[i], m);
    kp_wave_sync();
    part = 0.0f;
    for (uint32_t i = lane; i < W; i += 64u) part = __fmaf_rn(a[i], a[i], part);
    const float e1 = kp_lane_tree(part);
    for (uint32_t li = lane; li < nl; li += 64u) {
        const float* al = a + p.first_lag + li;                    // (i + lag <= W - 1 + last_lag = span - 1)
        float inner = 0.0f, e2 = 0.0f;
        for (uint32_t i = 0; i < W; i++) {
            const float zl = al[i];
            inner = __fmaf_rn(a[i], zl, inner);
            e2 = __fmaf_rn(zl, zl, e2);
        }
        const float norm = __fmul_rn(e1, e2);
        const float dp = sqrtf(__fadd_rn(norm, ballast)), dv = sqrtf(norm);
        nc[li] = dp != 0.0f ? inner / dp : 0.0f;
        nc[nl + li] = dv != 0.0f ? inner / dv : 0.0f;
    }
    kp_wave_sync();
    for (uint32_t s = lane; s < S; s += 64u) {
        uint32_t f0 = (uint32_t)p.tab.up_first[s];
        if (f0 + p.up_taps > nl) f0 = nl - p.up_taps;              // (the table never asks for it: up_taps <= n_lags, the host's check)
        const float* w = p.tab.up + (size_t)s * p.up_taps;
        float acc0 = 0.0f, acc1 = 0.0f;
        for (uint32_t k = 0; k < p.up_taps; k++) {
            acc0 = __fmaf_rn(w[k], nc[f0 + k], acc0);
            acc1 = __fmaf_rn(w[k], nc[nl + f0 + k], acc1);
        }
        o0[s] = acc0, o1[s] = acc1;
    }
}

__global__ __launch_bounds__(ALAC_KPITCH_DECODE_THREADS) void alac_kpitch_decode_kernel(alac_kpitch_decode_params p) {
    constexpr uint32_t TH = ALAC_KPITCH_DECODE_THREADS, WAVES = TH / 64, OWN = ALAC_KPITCH_MAX_STATES / TH;
    __shared__ float fwd_lds[2][ALAC_KPITCH_MAX_STATES];
    __shared__ float red_lds[WAVES];
    __shared__ uint32_t at_lds[WAVES];
    const uint32_t tid = threadIdx.x, S = p.n_states;
    const uint64_t plane = blockIdx.x, F = p.out_frames;
    const uint32_t row = (uint32_t)(plane / p.channels);
    uint64_t count;
    if (p.counts_are_frames) {
        count = kp_valid(p.valid, row, F);
    } else {
        count = alac_kpitch_frames(p.fr, kp_valid(p.valid, row, p.frames));
        if (count > F) count = F;
    }
    const bool process = (p.flags & ALAC_KPITCH_PROCESS) != 0u && p.out != nullptr;
    const uint32_t lines = alac_kpitch_lines(p.flags);
    float* raw = p.raw + plane * 2u * F;
    float* out = process ? p.out + plane * lines * F : nullptr;
    for (uint64_t t = count + tid; t < F; t += TH) {               // at and behind the line's count: zeros
        if (p.nccf) raw[t] = 0.0f, raw[F + t] = 0.0f;
        if (out)
            for (uint32_t l = 0; l < lines; l++) out[l * F + t] = 0.0f;
    }
    if (count == 0u) return;                                       // (the whole workgroup)
    if (p.nccf) {
        const float* np = p.nccf + plane * 2u * F * S;
        const float* nv = np + F * S;
        uint16_t* back = p.back + plane * F * S;
        const float factor = p.tab.head[0];
        float sl[OWN], val[OWN];
#pragma unroll
        for (uint32_t o = 0; o < OWN; o++) {
            const uint32_t i = tid + o * TH;
            sl[o] = i < S ? p.tab.sl[i] : 0.0f;
        }
        for (uint64_t t = 0; t < count; t++) {
            const float* prev = fwd_lds[(t + 1u) & 1u];
            float* next = fwd_lds[t & 1u];
            const float* n_t = np + t * S;
            float least = __builtin_inff();
#pragma unroll
            for (uint32_t o = 0; o < OWN; o++) {
                const uint32_t i = tid + o * TH;
                if (i >= S) continue;
                float best = 0.0f;
                if (t) {
                    uint32_t arg = 0u;
                    for (uint32_t j = 0; j < S; j++) {             // ascending sources: the lowest wins a tie
                        const int32_t dd = (int32_t)i - (int32_t)j;
                        const float cand = __fadd_rn(prev[j], __fmul_rn((float)(dd * dd), factor));
                        if (j == 0u || cand < best) best = cand, arg = j;
                    }
                    back[t * S + i] = (uint16_t)arg;
                    val[o] = __fadd_rn(best, kp_local(n_t[i], sl[o]));
                } else {
                    val[o] = kp_local(n_t[i], sl[o]);
                }
                if (val[o] < least) least = val[o];
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) {
                const float other = __shfl_xor(least, w, 64);
                if (other < least) least = other;
            }
            if ((tid & 63u) == 0u) red_lds[tid >> 6] = least;
            __syncthreads();                                       // (every read of prev lies in front of it)
#pragma unroll
            for (uint32_t w = 0; w < WAVES; w++)
                if (red_lds[w] < least) least = red_lds[w];
#pragma unroll
            for (uint32_t o = 0; o < OWN; o++) {
                const uint32_t i = tid + o * TH;
                if (i < S) next[i] = __fsub_rn(val[o], least);
            }
            __syncthreads();                                       // (next is read, red_lds written again, behind it)
        }
        // the first least cost of the last frame: a lane's states ascend, then lexicographic (smaller value, lower state)
        const float* last = fwd_lds[(count - 1u) & 1u];
        float best = __builtin_inff();
        uint32_t at = 0xFFFFFFFFu;
        for (uint32_t s = tid; s < S; s += TH) {
            const float x = last[s];
            if (at == 0xFFFFFFFFu || x < best) best = x, at = s;
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
            const float ob = __shfl_xor(best, w, 64);
            const uint32_t oa = (uint32_t)__shfl_xor((int)at, w, 64);
            if (oa != 0xFFFFFFFFu && (at == 0xFFFFFFFFu || ob < best || (ob == best && oa < at))) best = ob, at = oa;
        }
        if ((tid & 63u) == 0u) red_lds[tid >> 6] = best, at_lds[tid >> 6] = at;
        __syncthreads();                                           // (and the backpointers of the last frame are visible)
        if (tid == 0u) {
            for (uint32_t w = 1u; w < WAVES; w++) {
                const float ob = red_lds[w];
                const uint32_t oa = at_lds[w];
                if (oa != 0xFFFFFFFFu && (ob < best || (ob == best && oa < at))) best = ob, at = oa;
            }
            uint32_t s = at;                                       // the walk back, one dependent load a frame
            for (uint64_t t = count; t-- > 0u;) {
                raw[t] = nv[t * S + s];
                raw[F + t] = p.tab.hz[s];
                if (t) s = back[t * S + s];
            }
        }
        __syncthreads();                                           // (the raw track is visible to the epilogue)
    }
    if (!process) return;
    // the post-processing: a lane per frame, first the weight and the log-pitch of every frame, then the windows
    float* wp = p.work + plane * 2u * F;
    float* wl = wp + F;
    const float pitch_scale = p.tab.head[3], pov_scale = p.tab.head[4], pov_offset = p.tab.head[5], delta_scale = p.tab.head[6];
    const uint32_t l_pov = 0u, l_norm = (p.flags >> 1) & 1u, l_delta = l_norm + ((p.flags >> 2) & 1u), l_raw = l_delta + ((p.flags >> 3) & 1u);
    for (uint64_t t = tid; t < count; t += TH) {
        float n = raw[t];
        n = n < -1.0f ? -1.0f : (n > 1.0f ? 1.0f : n);
        const float lp = __fmul_rn(alac_pcen_log2(raw[F + t]), KP_LN2);
        const float nd = __builtin_fabsf(n), m1 = __fsub_rn(nd, 1.0f);
        const float e1 = __fmul_rn(5.4f, kp_exp(__fmul_rn(7.5f, m1)));
        const float e2 = __fmul_rn(2.0f, kp_exp(__fmul_rn(-10.0f, nd)));
        const float e3 = __fmul_rn(4.2f, kp_exp(__fmul_rn(20.0f, m1)));
        const float r = __fadd_rn(__fsub_rn(__fadd_rn(__fadd_rn(-5.2f, e1), __fmul_rn(4.8f, nd)), e2), e3);
        wp[t] = 1.0f / __fadd_rn(1.0f, kp_exp(-r));
        wl[t] = lp;
        if (p.flags & ALAC_KPITCH_POV) {
            const float pw = alac_pcen_exp2(__fmul_rn(0.15f, alac_pcen_log2(__fsub_rn(1.0001f, n))));
            out[l_pov * F + t] = __fadd_rn(__fmul_rn(pov_scale, __fsub_rn(pw, 1.0f)), pov_offset);
        }
        if (p.flags & ALAC_KPITCH_RAW) out[l_raw * F + t] = lp;
    }
    __syncthreads();
    for (uint64_t t = tid; t < count; t += TH) {
        const float lp = wl[t];
        if (p.flags & ALAC_KPITCH_NORM) {
            const uint64_t lo = t > p.left ? t - p.left : 0u, hi = t + p.right < count - 1u ? t + p.right : count - 1u;
            float sp = 0.0f, sl = 0.0f;
            for (uint64_t u = lo; u <= hi; u++) {                  // the window from its own elements, ascending
                const float pu = wp[u];
                sp = __fadd_rn(sp, pu);
                sl = __fadd_rn(sl, __fmul_rn(pu, wl[u]));
            }
            out[l_norm * F + t] = __fmul_rn(pitch_scale, __fsub_rn(lp, sl / sp));
        }
        if (p.flags & ALAC_KPITCH_DELTA) {
            const int64_t w = (int64_t)p.delta_window;
            float acc = 0.0f;
            for (int64_t j = -w; j <= w; j++) {
                int64_t u = (int64_t)t + j;
                u = u < 0 ? 0 : (u > (int64_t)count - 1 ? (int64_t)count - 1 : u);
                acc = __fadd_rn(acc, __fmul_rn(p.tab.dc[j + w], wl[u]));
            }
            out[l_delta * F + t] = __fmul_rn(delta_scale, acc);
        }
    }
}
