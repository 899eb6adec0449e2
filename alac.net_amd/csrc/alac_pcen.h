// alac_pcen.h -- the launch parameters, the thresholds, the grid and the two polynomials of the per-channel energy normalisation
// behind the features (alac_pcen.hip), shared with the C ABI (alacgpu_stages.hip).  The data is float32
// [rows, lines_per_row, line_stride] of which the first line_len elements of a line are data, as in alac_normalize.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A team of lanes takes a line in passes of ALAC_PCEN_CHUNK frames per lane, lane i of a pass at p0 the frames p0 + CHUNK i ..
// p0 + CHUNK i + CHUNK - 1, read as one vector load where all of them are below v.  Two teams, chosen from line_len alone:
//   line_len <= ALAC_PCEN_WAVE_MAX   a wave per line (a pass is 64 * CHUNK frames), ALAC_PCEN_WAVE_LINES lines per workgroup
//   above                            a workgroup of ALAC_PCEN_LINE_THREADS threads per line (a pass is LINE_THREADS * CHUNK frames)
// The order of the float32 operations, which the twin in alac.net_amd/pcen.py follows; every operation is rounded once, nothing
// is contracted, a = fl(1 - b), s[t] = fl(scale * x[t]):
//   a lane   from m = 0, A = 1 over its frames t < v ascending: m = fl(fl(a * m) + fl(b * s[t])), A = fl(A * a); at t = 0 instead
//            m = s[0], A = 0 (M[0] = s[0], whatever comes in).  m_k and A_k are m and A behind the lane's frame k; a frame at or
//            behind v changes neither.  The lane's map is (A, B) = (A_last, m_last): M behind its frames is A * M in front + B.
//   a wave   the inclusive scan of its 64 maps by __shfl_up, for d = 1, 2, 4, 8, 16, 32 and every lane >= d at once, with (A', B')
//            the map lane - d held in front of the step: B = fl(fl(A * B') + B), then A = fl(A * A').
//   a pass   with c the carry into the pass (0 into the first): into wave 0 goes c, into wave w + 1 fl(fl(A_w * c_w) + B_w) with
//            (A_w, B_w) lane 63's scanned map of wave w -- through LDS in the workgroup team --, and the carry into the next
//            pass is that of the last wave.  Into lane 0 of a wave goes C = c_w, into lane i > 0 C = fl(fl(A * c_w) + B) with (A, B)
//            the scanned map of lane i - 1.
//   a frame  M[t] = fl(fl(A_k * C) + m_k).
// The compression of a frame, with c = bias^power rounded once from float64 on the host, log2 and exp2 the two polynomials below:
//   u = fl(eps + M);  g = exp2(fl(-gain * log2(u)));  w = fl(fl(s * g) + bias);  y = fl(exp2(fl(power * log2(w))) - c).
constexpr uint32_t ALAC_PCEN_CHUNK = 4u;
constexpr int ALAC_PCEN_WAVE_THREADS = 256;
constexpr uint32_t ALAC_PCEN_WAVE_LINES = 4u;
constexpr uint32_t ALAC_PCEN_WAVE_MAX = 1024u;
constexpr int ALAC_PCEN_LINE_THREADS = 256;
constexpr uint32_t ALAC_PCEN_TABLE_ROWS = 5u;          // b, gain, bias, power, bias^power: [5, lines_per_param]
static_assert(ALAC_PCEN_WAVE_THREADS == 64 * (int)ALAC_PCEN_WAVE_LINES, "a wave per line");
static_assert(ALAC_PCEN_WAVE_MAX % (64u * ALAC_PCEN_CHUNK) == 0u, "the wave team's lines are whole passes at the threshold");

struct alac_pcen_params {
    const float* src;             // [lines, line_stride]
    float* out;                   // the same layout; may be src
    const int64_t* valid;         // [rows] or null: v = min(max(valid[r], 0), line_len), null: line_len
    const float* table;           // [ALAC_PCEN_TABLE_ROWS, lines_per_param] or null: the scalars below for every line
    uint64_t lines;               // rows * lines_per_row
    uint32_t lines_per_row, lines_per_param;
    uint64_t line_stride, line_len;
    float b, gain, bias, power, bias_pow, eps, scale;
    uint32_t stage;               // 0: y, 1: M
};

// The workgroups of a launch.  Neither kernel has dynamic LDS; the workgroup team holds its waves' maps in 8 bytes each.
__host__ __device__ inline uint64_t alac_pcen_grid(uint64_t lines, uint64_t line_len) {
    return line_len <= ALAC_PCEN_WAVE_MAX ? (lines + ALAC_PCEN_WAVE_LINES - 1u) / ALAC_PCEN_WAVE_LINES : lines;
}

// log2 of a float32, every operation written and rounded once (the division is the correctly rounded one): u = 2^e m with m in
// (sqrt(1/2), sqrt(2)] by the bits (a subnormal times 2^24 first), r = fl(fl(m - 1) / fl(m + 1)), z = fl(r * r),
// q = L0 + z (L1 + z (L2 + z (L3 + z L4))) by Horner's rule, log2 u = fl(e + fl(r * q)): the series of 2 atanh(r) / ln 2, whose
// next term is below 2e-9 of the sum.  +0 and -0 give -inf, +inf gives +inf, a negative number or a NaN gives NaN.
__host__ __device__ inline float alac_pcen_log2(float u) {
    if (!(u > 0.0f)) return u == 0.0f ? -__builtin_inff() : __builtin_nanf("");
    if (u == __builtin_inff()) return u;
    float e = 0.0f;
    if (u < 1.17549435e-38f) {
        u = u * 16777216.0f;
        e = -24.0f;
    }
    const uint32_t bits = __builtin_bit_cast(uint32_t, u);
    const uint32_t mant = bits & 0x7FFFFFu;
    const bool up = mant > 0x3504F3u;                  // above sqrt(2)'s mantissa: the exponent above, m below 1
    const float m = __builtin_bit_cast(float, mant | (up ? 0x3F000000u : 0x3F800000u));
    e = e + (float)((int32_t)(bits >> 23) - 127 + (up ? 1 : 0));
    const float r = (m - 1.0f) / (m + 1.0f);
    const float z = r * r;
    float q = 0.3205988980f;
    q = q * z + 0.4121985831f;
    q = q * z + 0.5770780164f;
    q = q * z + 0.9617966939f;
    q = q * z + 2.8853900818f;
    return e + r * q;
}

// 2^p of a float32, every operation written and rounded once: k = p rounded to the nearest integer, ties to even, f = p - k
// (exact), q = 1 + f (E1 + f (E2 + ... + f E7)) by Horner's rule with E_j = ln(2)^j / j!, and fl(fl(q * 2^k1) * 2^k2) with
// k1 = floor(k / 2), k2 = k - k1: the first product is exact, the second rounds where the result is subnormal.  p >= 128 gives
// +inf, p < -150 gives 0, a NaN gives NaN.
__host__ __device__ inline float alac_pcen_exp2(float p) {
    if (!(p < 128.0f)) return p != p ? p : __builtin_inff();
    if (p < -150.0f) return 0.0f;
    const float k = __builtin_rintf(p);
    const float f = p - k;
    float q = 1.5252734e-05f;
    q = q * f + 1.5403530e-04f;
    q = q * f + 1.3333558e-03f;
    q = q * f + 9.6181291e-03f;
    q = q * f + 5.5504109e-02f;
    q = q * f + 2.4022651e-01f;
    q = q * f + 6.9314718e-01f;
    q = q * f + 1.0f;
    const int32_t ki = (int32_t)k, k1 = ki >> 1, k2 = ki - k1;
    const float s1 = __builtin_bit_cast(float, (uint32_t)(k1 + 127) << 23), s2 = __builtin_bit_cast(float, (uint32_t)(k2 + 127) << 23);
    return (q * s1) * s2;
}

__global__ void alac_pcen_wave_kernel(alac_pcen_params p);
__global__ void alac_pcen_line_kernel(alac_pcen_params p);
