// alac_features.hip -- log-mel features of decoded PCM in one launch (alacgpu_logmel_device): framing with reflection, the
// window, the DFT as a GEMM on the exact-f32 MFMA, power, the mel projection and the log (alac.net_amd/features.py states the
// mathematics).  The tile body is alac_features.h's, which describes it; what is the log-mel kernel's own:
//   * frames are centred, K = n_fft, and the span load reflects once at either end of the signal
//   * the B operand is window[n] * x[t hop + n], one rounding
//   * max(M, floor) and the natural or decimal log, by log_mode
#include "alac_features.h"

namespace {

constexpr uint32_t AHEAD = 8u;   // k-steps (of two taps) whose basis fragments are loaded ahead

}  // namespace

__global__ __launch_bounds__(ALAC_FEATURES_THREADS) void alac_logmel_kernel(alac_features_params p) {
    extern __shared__ __align__(16) float lds[];
    const alac_stft_mel_tile c(p, lds, 0u);
    const int64_t L = (int64_t)p.frames;
    // the span: reflected once at either end; what one reflection does not bring inside (frames behind the last one of a short
    // tile; odd n_fft at L = n_fft / 2 + 1) is zero and nothing is read for it
    c.load(-(int64_t)(p.n_fft / 2u), [&](int64_t g) {
        if (g < 0) g = -g;
        else if (g >= L) g = 2 * (L - 1) - g;
        return (g >= 0 && g < L) ? c.src[g] : 0.0f;
    });
    c.transform<AHEAD>([&](uint32_t n, uint32_t q, uint32_t r) { return c.win[n] * c.xs[c.xbase + n + c.skew * q]; },
                       [](float re, float im) { return alac_stft_mel_power(re, im); },
                       [&](float v) {
                           if (p.log_mode != ALAC_FEATURES_LOG_NONE) {
                               v = v < p.floor ? p.floor : v;     // (a NaN stays a NaN, as in np.maximum and torch.clamp)
                               v = p.log_mode == ALAC_FEATURES_LOG_LN ? logf(v) : log10f(v);
                           }
                           return v;
                       });
}
