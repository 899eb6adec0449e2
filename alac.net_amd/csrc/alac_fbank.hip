// alac_fbank.hip -- Kaldi filterbank features of decoded PCM in one launch (alacgpu_fbank_device): framing without centring
// (snip_edges) or with Kaldi's reflection, the frame's mean, pre-emphasis, the window, the zero-padded DFT as a GEMM on the
// exact-f32 MFMA, power, the mel projection and the log (alac.net_amd/fbank.py states the mathematics and the float32 order).
//
// The shape is the log-mel kernel's (alac_features.hip): a workgroup of four waves owns a tile of up to 32 consecutive frames of
// one plane, loads the span of signal they cover, (tile - 1) hop + win samples, into LDS once, and computes D = basis^T .
// frames^T on v_mfma_f32_32x32x2_f32 with the frame on the lanes and the bin in the registers, two accumulators per block of 32
// bins over K = win.  Zero-padding win to n_fft costs nothing: the basis has win rows at angles 2 pi n k / n_fft, its leading
// dimension is 2 n_bins of n_fft.  The basis is read from global memory as fragments through L2, eight k-steps ahead; the
// epilogue -- power (or its root), the mel sums between rounds of eight blocks, floor, log, store -- stays on chip.  Every
// element of `out` has exactly one writer; no atomics; all loads and stores are plain vector ones.
//
// What is new:
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
// This file is compiled without contraction and with the correctly rounded division and root: every operation is the one
// written.
#include "alac_fbank.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t AHEAD = 8u;   // k-steps (of two taps) whose basis fragments are loaded ahead

static_assert(ALAC_FEATURES_THREADS == ALAC_FEATURES_TILE * ALAC_FBANK_MEAN_PARTIALS, "eight threads sum a frame's mean");

}  // namespace

__global__ __launch_bounds__(ALAC_FEATURES_THREADS) void alac_fbank_kernel(alac_fbank_params p) {
    extern __shared__ __align__(16) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t t = tid & 31u;             // the frame of the tile: the lane's column of B and of D
    const uint32_t h = (tid >> 5) & 1u;       // the lane's k of a k-step, and its half of D's rows
    const uint32_t wave = ((tid >> 6) + blockIdx.x) & 3u;
    const uint32_t win_n = p.win, hop = p.hop, n_mels = p.n_mels;
    const uint32_t n_bins = p.n_fft / 2u + 1u;
    const uint32_t ldb = 2u * n_bins;
    const uint32_t n_blocks = (n_bins + ALAC_FEATURES_BLOCK - 1u) / ALAC_FEATURES_BLOCK;
    const alac_fbank_lds lay = alac_fbank_lds_layout(win_n, p.n_fft, hop, n_mels);
    float* const win = lds;
    float* const mel = win + lay.window;
    float* const pw = mel + lay.mel;
    float* const mean = pw + lay.power;
    float* const xs = mean + lay.mean;
    const uint32_t skew = alac_features_skew(hop);

    const uint32_t tile_i = blockIdx.x % p.tiles;
    const uint64_t plane = blockIdx.x / p.tiles;
    const uint64_t t0 = (uint64_t)tile_i * p.tile;
    const uint64_t left = p.out_frames - t0;
    const uint32_t nt = left < p.tile ? (uint32_t)left : p.tile;   // the tile's frames
    const float* const src = p.src + plane * p.src_stride;
    const int64_t L = (int64_t)p.frames;
    const bool snip = (p.flags & ALAC_FBANK_SNIP_EDGES) != 0u;

    for (uint32_t i = tid; i < win_n; i += ALAC_FEATURES_THREADS) win[i] = p.window[i];
    for (uint32_t i = tid; i < lay.mel; i += ALAC_FEATURES_THREADS) mel[i] = 0.0f;
    // the span: sample s_lo + idx, scaled.  snip_edges: the frames of the row lie inside it, what a short tile's missing frames
    // would cover behind L is zero and not read; else Kaldi's reflection, which brings every index inside
    const int64_t s_lo = (int64_t)(t0 * hop) + (snip ? 0 : (int64_t)(hop / 2u) - (int64_t)(win_n / 2u));
    const uint32_t span = (p.tile - 1u) * hop + win_n;
    for (uint32_t idx = tid; idx < span; idx += ALAC_FEATURES_THREADS) {
        int64_t g = s_lo + (int64_t)idx;
        if (!snip && (g < 0 || g >= L)) {
            int64_t m = g % (2 * L);
            if (m < 0) m += 2 * L;
            g = m < L ? m : 2 * L - 1 - m;
        }
        float v = 0.0f;
        if (g >= 0 && g < L) v = p.scale * src[g];
        xs[idx + skew * (idx / hop)] = v;
    }
    __syncthreads();

    // the means: thread (frame f, j) sums the taps j, j + 8 ... of frame f, then the tree over j
    {
        const uint32_t f = tid / ALAC_FBANK_MEAN_PARTIALS, j = tid % ALAC_FBANK_MEAN_PARTIALS;
        float part = 0.0f;
        if ((p.flags & ALAC_FBANK_REMOVE_DC) != 0u && f < nt) {
            const float* const xf = xs + f * (hop + skew);
            for (uint32_t n = j; n < win_n; n += ALAC_FBANK_MEAN_PARTIALS) part += xf[n + (skew ? n / hop : 0u)];
        }
        part += __shfl_xor(part, 1);
        part += __shfl_xor(part, 2);
        part += __shfl_xor(part, 4);
        if (j == 0u) mean[f] = part / (float)win_n;      // (0 without remove_dc_offset: s - 0 is s)
    }
    __syncthreads();

    const bool frame_ok = t < nt;
    const uint32_t xbase = frame_ok ? t * (hop + skew) : 0u;
    const float mu = mean[t];
    const float c = p.preemphasis;
    const bool pre = c != 0.0f;
    const bool root = (p.flags & ALAC_FBANK_USE_POWER) == 0u;
    const uint32_t pairs = win_n / 2u;        // k-steps with both taps inside

    // B[n][t] = window[n] * (d[n] - c d[n - 1]), d = s - mu, d[-1] = d[0]; tap n = q hop + r of the lane's frame
    const auto tap = [&](uint32_t n, uint32_t q, uint32_t r) -> float {
        const uint32_t pos = xbase + n + skew * q;
        const uint32_t back = n == 0u ? 0u : 1u + ((skew != 0u && r == 0u) ? 1u : 0u);   // (over the padding in front of a hop)
        const float dn = xs[pos] - mu;
        const float dp = xs[pos - back] - mu;
        const float y = pre ? __builtin_fmaf(-c, dp, dn) : dn;
        return win[n] * y;
    };

    for (uint32_t round0 = 0; round0 < n_blocks; round0 += ALAC_FEATURES_ROUND_BLOCKS) {
        const uint32_t round_end = round0 + ALAC_FEATURES_ROUND_BLOCKS < n_blocks ? round0 + ALAC_FEATURES_ROUND_BLOCKS : n_blocks;
        for (uint32_t blk = round0 + wave; blk < round_end; blk += 4u) {
            uint32_t col = blk * ALAC_FEATURES_BLOCK + t;     // (t: the lane's row of A as well)
            col = col < n_bins ? col : n_bins - 1u;
            const float* a_re = p.basis + col + (size_t)h * ldb;
            const float* a_im = a_re + n_bins;
            const size_t a_step = 2u * (size_t)ldb;
            f32x16 re = {}, im = {};
            // the lane's tap n = 2 s + h = q hop + r, kept as q and r for the skew
            uint32_t n = h, q = 0, r = h;
            if (r >= hop) {   // hop 1 (no skew: q and r are not used)
                q = r;
                r = 0;
            }
            float ar[AHEAD], ai[AHEAD];
            uint32_t s = 0;
            for (; s + AHEAD <= pairs; s += AHEAD) {
#pragma unroll
                for (uint32_t u = 0; u < AHEAD; ++u) {
                    ar[u] = a_re[u * a_step];
                    ai[u] = a_im[u * a_step];
                }
                a_re += AHEAD * a_step;
                a_im += AHEAD * a_step;
#pragma unroll
                for (uint32_t u = 0; u < AHEAD; ++u) {
                    const float b = frame_ok ? tap(n, q, r) : 0.0f;
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[u], b, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[u], b, im, 0, 0, 0);
                    n += 2u;
                    r += 2u;
                    if (r >= hop) {
                        r -= hop;
                        q += 1u;
                    }
                }
            }
            // what is left: up to AHEAD - 1 whole k-steps and, for an odd win, one with the tap of h = 1 outside
            for (; 2u * s < win_n; ++s) {
                const bool ok = n < win_n;
                const float vr = ok ? a_re[0] : 0.0f;
                const float vi = ok ? a_im[0] : 0.0f;
                const float b = (ok && frame_ok) ? tap(n, q, r) : 0.0f;
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(vr, b, re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(vi, b, im, 0, 0, 0);
                if (2u * s + 2u < win_n) {      // (the next step exists: its row h = 0 is inside the basis)
                    a_re += a_step;
                    a_im += a_step;
                }
                n += 2u;
                r += 2u;
                if (r >= hop) {
                    r -= hop;
                    q += 1u;
                }
            }
            // D's register j of this lane is bin (j & 3) + 8 (j >> 2) + 4 h of the block, frame t
            float* const dst = pw + (blk - round0) * (ALAC_FEATURES_BLOCK * ALAC_FEATURES_TILE) + t;
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                const uint32_t row = (j & 3u) + 8u * (j >> 2) + 4u * h;
                const float pwr = __builtin_fmaf(re[j], re[j], im[j] * im[j]);
                dst[row * ALAC_FEATURES_TILE] = root ? sqrtf(pwr) : pwr;
            }
        }
        __syncthreads();
        // the round's bins into the mel sums: thread (m, t) continues its chain
        const uint32_t kb = round0 * ALAC_FEATURES_BLOCK;
        const uint32_t ke = round_end * ALAC_FEATURES_BLOCK < n_bins ? round_end * ALAC_FEATURES_BLOCK : n_bins;
        for (uint32_t m = tid >> 5; m < n_mels; m += ALAC_FEATURES_THREADS / 32u) {
            const float* const f = p.fb + (size_t)m * n_bins;
            const float* const pk = pw + t;
            float acc = mel[m * ALAC_FEATURES_TILE + t];
#pragma unroll 4
            for (uint32_t k = kb; k < ke; ++k) acc = __builtin_fmaf(f[k], pk[(k - kb) * ALAC_FEATURES_TILE], acc);
            mel[m * ALAC_FEATURES_TILE + t] = acc;
        }
        __syncthreads();
    }

    // (a thread reads the sums it wrote itself)
    if (frame_ok) {
        float* const out = p.out + plane * n_mels * p.out_frames + t0 + t;
        for (uint32_t m = tid >> 5; m < n_mels; m += ALAC_FEATURES_THREADS / 32u) {
            float v = mel[m * ALAC_FEATURES_TILE + t];
            if ((p.flags & ALAC_FBANK_LOG) != 0u) {
                v = v < ALAC_FBANK_FLOOR ? ALAC_FBANK_FLOOR : v;     // (a NaN stays a NaN, as in np.maximum and torch.clamp)
                v = logf(v);
            }
            out[(uint64_t)m * p.out_frames] = v;
        }
    }
}
