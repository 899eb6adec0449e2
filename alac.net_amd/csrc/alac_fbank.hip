// alac_fbank.hip -- Kaldi filterbank features of decoded PCM in one launch (alacgpu_fbank_device): framing without centring
// (snip_edges) or with Kaldi's reflection, the frame's mean, pre-emphasis, the window, the zero-padded DFT as a GEMM on the
// exact-f32 MFMA, power, the mel projection and the log (alac.net_amd/fbank.py states the mathematics and the float32 order).
// The tile body is alac_features.h's, which describes it, with K = win; what is the fbank kernel's own:
//   * the span load scales the sample (s = scale * x, one rounding) and, without snip_edges, reflects an index outside
//     0 .. L in closed form: m = g mod 2 L (floored), then m or 2 L - 1 - m.  Nothing outside [0, L) of a plane is read.
//   * a pass over the span computes the mean of each frame: eight threads per frame, thread j the taps j, j + 8 ... in
//     ascending order, then ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)) by three exchanges between lanes, divided by win.
//   * the B operand belongs to a frame, not to a sample -- a sample has another mean and another predecessor rule in every
//     frame it is part of -- so it is evaluated as it is read: window[n] * fma(-c, s[n - 1] - mu, s[n] - mu) from two
//     neighbouring LDS words and the lane's own mean (the lane is the frame: the mean is a register), tap 0 its own
//     predecessor.  That is one more LDS read and four more vector instructions per tap, issued beside two MFMAs of 64 cycles
//     each, against 32 win floats of LDS for frames preprocessed once (51 KB at 400, more than a CU has at 2048, and a second
//     path for it).
//   * the root of the power without use_power; the floor 2^-23 and the natural log by flag
// This file is compiled without contraction and with the correctly rounded division and root: every operation is the one
// written.
#include "alac_fbank.h"

namespace {

constexpr uint32_t AHEAD = 8u;   // k-steps (of two taps) whose basis fragments are loaded ahead

static_assert(ALAC_FEATURES_THREADS == ALAC_FEATURES_TILE * ALAC_FBANK_MEAN_PARTIALS, "eight threads sum a frame's mean");

}  // namespace

__global__ __launch_bounds__(ALAC_FEATURES_THREADS) void alac_fbank_kernel(alac_fbank_params p) {
    extern __shared__ __align__(16) float lds[];
    const alac_stft_mel_tile c(p, lds, ALAC_FBANK_LDS_EXTRA);
    float* const mean = c.extra;
    const uint32_t win_n = p.taps, hop = p.hop, skew = c.skew;
    const int64_t L = (int64_t)p.frames;
    const bool snip = (p.flags & ALAC_FBANK_SNIP_EDGES) != 0u;

    // the span, scaled.  snip_edges: the frames of the row lie inside it, what a short tile's missing frames would cover behind
    // L is zero and not read; else Kaldi's reflection, which brings every index inside
    c.load(snip ? 0 : (int64_t)(hop / 2u) - (int64_t)(win_n / 2u), [&](int64_t g) {
        if (!snip && (g < 0 || g >= L)) {
            int64_t m = g % (2 * L);
            if (m < 0) m += 2 * L;
            g = m < L ? m : 2 * L - 1 - m;
        }
        return (g >= 0 && g < L) ? p.scale * c.src[g] : 0.0f;
    });

    // the means: thread (frame f, j) sums the taps j, j + 8 ... of frame f, then the tree over j
    {
        const uint32_t f = c.tid / ALAC_FBANK_MEAN_PARTIALS, j = c.tid % ALAC_FBANK_MEAN_PARTIALS;
        float part = 0.0f;
        if ((p.flags & ALAC_FBANK_REMOVE_DC) != 0u && f < c.nt) {
            const float* const xf = c.xs + f * (hop + skew);
            for (uint32_t n = j; n < win_n; n += ALAC_FBANK_MEAN_PARTIALS) part += xf[n + (skew ? n / hop : 0u)];
        }
        part += __shfl_xor(part, 1);
        part += __shfl_xor(part, 2);
        part += __shfl_xor(part, 4);
        if (j == 0u) mean[f] = part / (float)win_n;      // (0 without remove_dc_offset: s - 0 is s)
    }
    __syncthreads();

    const float mu = mean[c.t];
    const float pre_c = p.preemphasis;
    const bool pre = pre_c != 0.0f;
    const bool root = (p.flags & ALAC_FBANK_USE_POWER) == 0u;
    c.transform<AHEAD>(
        // B[n][t] = window[n] * (d[n] - c d[n - 1]), d = s - mu, d[-1] = d[0]; tap n = q hop + r of the lane's frame
        [&](uint32_t n, uint32_t q, uint32_t r) {
            const uint32_t pos = c.xbase + n + skew * q;
            const uint32_t back = n == 0u ? 0u : 1u + ((skew != 0u && r == 0u) ? 1u : 0u);   // (over the padding in front of a hop)
            const float dn = c.xs[pos] - mu;
            const float dp = c.xs[pos - back] - mu;
            const float y = pre ? __builtin_fmaf(-pre_c, dp, dn) : dn;
            return c.win[n] * y;
        },
        [&](float re, float im) {
            const float pwr = alac_stft_mel_power(re, im);
            return root ? sqrtf(pwr) : pwr;
        },
        [&](float v) {
            if ((p.flags & ALAC_FBANK_LOG) != 0u) {
                v = v < ALAC_FBANK_FLOOR ? ALAC_FBANK_FLOOR : v;     // (a NaN stays a NaN, as in np.maximum and torch.clamp)
                v = logf(v);
            }
            return v;
        });
}
