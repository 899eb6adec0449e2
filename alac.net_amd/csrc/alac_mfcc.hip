// alac_mfcc.hip -- Kaldi MFCC features of decoded PCM in one launch (alacgpu_mfcc_device): the fbank kernel's framing, mean,
// pre-emphasis, window, DFT and mel projection (alac_fbank.hip describes them; the tile body is alac_features.h's), and behind
// the last round, on chip, what is the MFCC kernel's own (alac.net_amd/mfcc.py states the mathematics and the float32 order):
//   * the frame's log energy, beside the mean: the eight threads that sum a frame's mean all hold the sum after the three
//     exchanges, so each forms mu itself and goes straight on to its partial of the energy -- taps j, j + 8 ... in ascending
//     order, part = fma(e, e, part), e the frame after scale and mean (raw_energy) or the windowed frame, evaluated as the B
//     operand is -- and the same tree.  No barrier between the two; the energies are 32 more floats of LDS.
//   * the epilogue: thread (m, t) replaces its mel sum in LDS by ln(max(M, 2^-23)); behind one barrier thread (c, t) runs the
//     chain C[c] = sum over m of dct[c, m] * lm[m], fused multiply-adds in ascending m from zero, multiplies by lifter[c] and
//     stores frame t0 + t of cepstrum c (with use_energy cepstrum 0 is the energy, un-liftered): lane t of 32 stores frame
//     t0 + t, neighbouring lanes neighbouring frames.  n_ceps * n_mels fused multiply-adds per frame against 2 * win * n_bins
//     for the DFT: VALU work, and the chain's order is the specification.
// Every element of `out` has one writer; no atomics; all loads and stores are plain vector ones.  This file is compiled as
// alac_fbank.o is, without contraction and with the correctly rounded division and root: every operation is the one written.
#include "alac_mfcc.h"

namespace {

constexpr uint32_t AHEAD = 8u;   // k-steps (of two taps) whose basis fragments are loaded ahead

static_assert(ALAC_FEATURES_THREADS == ALAC_FEATURES_TILE * ALAC_FBANK_MEAN_PARTIALS, "eight threads sum a frame's mean");

}  // namespace

__global__ __launch_bounds__(ALAC_FEATURES_THREADS) void alac_mfcc_kernel(alac_mfcc_params p) {
    extern __shared__ __align__(16) float lds[];
    const alac_stft_mel_tile c(p, lds, ALAC_MFCC_LDS_EXTRA);
    float* const mean = c.extra;
    float* const energy = c.extra + ALAC_FEATURES_TILE;
    const uint32_t win_n = p.taps, hop = p.hop, skew = c.skew;
    const int64_t L = (int64_t)p.frames;
    const bool snip = (p.flags & ALAC_FBANK_SNIP_EDGES) != 0u;
    const float pre_c = p.preemphasis;
    const bool pre = pre_c != 0.0f;

    // the span, scaled, as the fbank kernel loads it: nothing outside [0, L) of a plane is read
    c.load(snip ? 0 : (int64_t)(hop / 2u) - (int64_t)(win_n / 2u), [&](int64_t g) {
        if (!snip && (g < 0 || g >= L)) {
            int64_t m = g % (2 * L);
            if (m < 0) m += 2 * L;
            g = m < L ? m : 2 * L - 1 - m;
        }
        return (g >= 0 && g < L) ? p.scale * c.src[g] : 0.0f;
    });

    // the means and the energies: thread (frame f, j) sums the taps j, j + 8 ... of frame f, then the tree over j, twice
    {
        const uint32_t f = c.tid / ALAC_FBANK_MEAN_PARTIALS, j = c.tid % ALAC_FBANK_MEAN_PARTIALS;
        const bool has = f < c.nt;
        const float* const xf = c.xs + f * (hop + skew);
        float part = 0.0f;
        if ((p.flags & ALAC_FBANK_REMOVE_DC) != 0u && has)
            for (uint32_t n = j; n < win_n; n += ALAC_FBANK_MEAN_PARTIALS) part += xf[n + (skew ? n / hop : 0u)];
        part += __shfl_xor(part, 1);
        part += __shfl_xor(part, 2);
        part += __shfl_xor(part, 4);
        const float mu = part / (float)win_n;            // (every j holds the sum; 0 without remove_dc_offset: s - 0 is s)
        if (j == 0u) mean[f] = mu;
        if ((p.flags & ALAC_MFCC_USE_ENERGY) != 0u) {
            const bool raw = (p.flags & ALAC_MFCC_RAW_ENERGY) != 0u;
            float sq = 0.0f;
            if (has)
                for (uint32_t n = j; n < win_n; n += ALAC_FBANK_MEAN_PARTIALS) {
                    const float dn = xf[n + (skew ? n / hop : 0u)] - mu;
                    float e = dn;
                    if (!raw) {
                        const uint32_t b = n == 0u ? 0u : n - 1u;
                        const float dp = xf[b + (skew ? b / hop : 0u)] - mu;
                        e = c.win[n] * (pre ? __builtin_fmaf(-pre_c, dp, dn) : dn);
                    }
                    sq = __builtin_fmaf(e, e, sq);
                }
            sq += __shfl_xor(sq, 1);
            sq += __shfl_xor(sq, 2);
            sq += __shfl_xor(sq, 4);
            if (j == 0u) {
                float v = sq < ALAC_FBANK_FLOOR ? ALAC_FBANK_FLOOR : sq;     // (a NaN stays a NaN)
                v = logf(v);
                energy[f] = v < p.log_energy_floor ? p.log_energy_floor : v;
            }
        }
    }
    __syncthreads();

    const float mu = mean[c.t];
    const bool root = (p.flags & ALAC_FBANK_USE_POWER) == 0u;
    c.rounds<AHEAD>(
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
        });

    // the log-mel vector over the mel sums (thread (m, t) wrote the sum it now replaces), then the projection
    const uint32_t n_mels = p.n_mels, n_ceps = p.n_ceps;
    for (uint32_t m = c.tid >> 5; m < n_mels; m += ALAC_FEATURES_THREADS / 32u) {
        float v = c.mel[m * ALAC_FEATURES_TILE + c.t];
        v = v < ALAC_FBANK_FLOOR ? ALAC_FBANK_FLOOR : v;                     // (a NaN stays a NaN)
        c.mel[m * ALAC_FEATURES_TILE + c.t] = logf(v);
    }
    __syncthreads();
    if (c.frame_ok) {
        const bool use_energy = (p.flags & ALAC_MFCC_USE_ENERGY) != 0u;
        const float* const lm = c.mel + c.t;
        float* const out = p.out + c.plane * n_ceps * p.out_frames + c.t0 + c.t;
        for (uint32_t k = c.tid >> 5; k < n_ceps; k += ALAC_FEATURES_THREADS / 32u) {
            const float* const row = p.dct + (size_t)k * n_mels;
            float acc = 0.0f;
#pragma unroll 4
            for (uint32_t m = 0; m < n_mels; ++m) acc = __builtin_fmaf(row[m], lm[m * ALAC_FEATURES_TILE], acc);
            const float v = p.lifter[k] * acc;
            out[(uint64_t)k * p.out_frames] = (use_energy && k == 0u) ? energy[c.t] : v;
        }
    }
}
