// alac_features.hip -- log-mel features of decoded PCM in one launch (alacgpu_logmel_device): framing with reflection, the
// window, the DFT as a GEMM on the exact-f32 MFMA, power, the mel projection and the log (alac.net_amd/features.py states the
// mathematics).
//
// A workgroup of four waves owns a tile of 32 consecutive frames of one plane (row, channel).  It loads the span of signal
// those frames cover, (tile - 1) hop + n_fft samples, into LDS once: neighbouring lanes load neighbouring samples, and the
// reflection at both ends of the signal happens on that load -- nothing outside [0, frames) is read, whatever the stride.
//
// The DFT is D = basis^T . frames^T on v_mfma_f32_32x32x2_f32: the A operand is a block of 32 basis columns (bins), the B
// operand the 32 frames of the tile, so a result's frame index is on the lanes and its bin in the registers.  A wave takes a
// block of 32 bins at a time and runs two accumulators over K = n_fft, the block's cosine columns and its sine columns; they
// share the B operand, window[n] * x[t hop + n], one rounding, multiplied as it is read from LDS (a sample belongs to
// n_fft / hop frames with another window tap in each, so the product cannot be stored with the span).  An odd n_fft gets
// one zero k, bins past n_bins are computed on a clamped column and never used.  The MFMA is a k-ordered chain of f32 fused
// multiply-adds: the bound of features.py rests on that.
//
// Where the basis lives: in global memory, read as fragments through L2.  It is n_fft x 2 n_bins floats -- 643 KB at n_fft
// 400, 16.8 MB at 2048 -- and a workgroup uses every element of it exactly once, each by one wave: there is nothing for LDS to
// share between the waves, so streaming it through LDS would add a store, a barrier and a load to every element for no reuse.
// A fragment load is two runs of 32 neighbouring floats per wave, full 128-byte lines; per k-step a wave fetches 512 bytes
// against 128 cycles of MFMA, 16 bytes per clock per CU at full rate, a quarter of what L2 gives a CU.  At n_fft 400 the whole
// basis stays in L2 (4 MB per XCD) across the launch.  The loads of the next eight k-steps are issued ahead of the MFMAs of the
// current eight.
//
// The epilogue stays on chip.  A wave squares its block (P = re^2 + im^2, both in the same lane and register) into LDS,
// [bin][frame]; after a round of eight blocks all threads add the round's bins to the mel sums, M[m][t] += fb[m][k] P[k][t],
// ascending k, f32 fused multiply-adds on the VALU (the projection is a tenth of the DFT's arithmetic; fb is dense, the
// caller's), the sums in LDS between rounds.  Then max(M, floor), the log, and the store: lane t of 32 stores frame t0 + t of
// mel m, neighbouring lanes neighbouring frames.  Every element of `out` has exactly one writer; no atomics; all loads and
// stores are plain vector ones.
#include "alac_features.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t AHEAD = 8u;   // k-steps (of two taps) whose basis fragments are loaded ahead

}  // namespace

__global__ __launch_bounds__(ALAC_FEATURES_THREADS) void alac_logmel_kernel(alac_features_params p) {
    extern __shared__ __align__(16) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t t = tid & 31u;             // the frame of the tile: the lane's column of B and of D
    const uint32_t h = (tid >> 5) & 1u;       // the lane's k of a k-step, and its half of D's rows
    const uint32_t wave = ((tid >> 6) + blockIdx.x) & 3u;   // rotated: the wave that gets the odd block out is another SIMD's in the next workgroup
    const uint32_t n_fft = p.n_fft, hop = p.hop, n_mels = p.n_mels;
    const uint32_t n_bins = n_fft / 2u + 1u;
    const uint32_t ldb = 2u * n_bins;
    const uint32_t n_blocks = (n_bins + ALAC_FEATURES_BLOCK - 1u) / ALAC_FEATURES_BLOCK;
    const alac_features_lds lay = alac_features_lds_layout(n_fft, hop, n_mels);
    float* const win = lds;
    float* const mel = win + lay.window;
    float* const pw = mel + lay.mel;
    float* const xs = pw + lay.power;
    const uint32_t skew = alac_features_skew(hop);

    const uint32_t tile_i = blockIdx.x % p.tiles;
    const uint64_t plane = blockIdx.x / p.tiles;
    const uint64_t t0 = (uint64_t)tile_i * p.tile;
    const uint64_t left = p.out_frames - t0;
    const uint32_t nt = left < p.tile ? (uint32_t)left : p.tile;   // the tile's frames
    const float* const src = p.src + plane * p.src_stride;
    const int64_t L = (int64_t)p.frames;

    for (uint32_t i = tid; i < n_fft; i += ALAC_FEATURES_THREADS) win[i] = p.window[i];
    for (uint32_t i = tid; i < lay.mel; i += ALAC_FEATURES_THREADS) mel[i] = 0.0f;
    // the span: sample s_lo + idx, reflected once at either end; what one reflection does not bring inside (frames behind the
    // last one of a short tile; odd n_fft at L = n_fft / 2 + 1) is zero and nothing is read for it
    const int64_t s_lo = (int64_t)(t0 * hop) - (int64_t)(n_fft / 2u);
    const uint32_t span = (p.tile - 1u) * hop + n_fft;
    for (uint32_t idx = tid; idx < span; idx += ALAC_FEATURES_THREADS) {
        int64_t g = s_lo + (int64_t)idx;
        if (g < 0) g = -g;
        else if (g >= L) g = 2 * (L - 1) - g;
        float v = 0.0f;
        if (g >= 0 && g < L) v = src[g];
        xs[idx + skew * (idx / hop)] = v;
    }
    __syncthreads();

    const bool frame_ok = t < nt;
    const uint32_t xbase = frame_ok ? t * (hop + skew) : 0u;
    const uint32_t pairs = n_fft / 2u;        // k-steps with both taps inside

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
            if (r >= hop) {   // hop 1 (no skew: q is not used)
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
                    const float b = frame_ok ? win[n] * xs[xbase + n + skew * q] : 0.0f;
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
            // what is left: up to AHEAD - 1 whole k-steps and, for an odd n_fft, one with the tap of h = 1 outside
            for (; 2u * s < n_fft; ++s) {
                const bool ok = n < n_fft;
                const float vr = ok ? a_re[0] : 0.0f;
                const float vi = ok ? a_im[0] : 0.0f;
                const float b = (ok && frame_ok) ? win[n] * xs[xbase + n + skew * q] : 0.0f;
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(vr, b, re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(vi, b, im, 0, 0, 0);
                if (2u * s + 2u < n_fft) {      // (the next step exists: its row h = 0 is inside the basis)
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
                dst[row * ALAC_FEATURES_TILE] = __builtin_fmaf(re[j], re[j], im[j] * im[j]);
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
            if (p.log_mode != ALAC_FEATURES_LOG_NONE) {
                v = v < p.floor ? p.floor : v;     // (a NaN stays a NaN, as in np.maximum and torch.clamp)
                v = p.log_mode == ALAC_FEATURES_LOG_LN ? logf(v) : log10f(v);
            }
            out[(uint64_t)m * p.out_frames] = v;
        }
    }
}
