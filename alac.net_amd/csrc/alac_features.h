// alac_features.h -- the fused STFT + mel kernels: the launch parameters and the LDS layout, shared with the C ABI
// (alacgpu_stages.hip), and the tile body (alac_stft_mel_tile) that the log-mel kernel (alac_features.hip), the Kaldi fbank
// kernel (alac_fbank.hip, alac_fbank.h) and the Kaldi MFCC kernel (alac_mfcc.hip, alac_mfcc.h) are made of.  A kernel supplies what is its own -- how a sample of the span is
// read, the B operand of a tap, what becomes of a bin's power, what becomes of a mel sum -- as lambdas, which inline; the loop
// over K, its remainder, the scatter of D and the mel sums exist here and nowhere else.
//
// A workgroup of four waves owns a tile of 32 consecutive frames of one plane (row, channel).  It loads the span of signal
// those frames cover, (tile - 1) hop + taps samples, into LDS once: neighbouring lanes load neighbouring samples, and what
// happens at both ends of the signal happens on that load -- nothing outside [0, frames) is read, whatever the stride.
//
// The DFT is D = basis^T . frames^T on v_mfma_f32_32x32x2_f32: the A operand is a block of 32 basis columns (bins), the B
// operand the 32 frames of the tile, so a result's frame index is on the lanes and its bin in the registers.  A wave takes a
// block of 32 bins at a time and runs two accumulators over K = taps (log-mel: n_fft; fbank: the window, whose zero-padding to
// n_fft costs nothing -- the basis has taps rows at angles 2 pi n k / n_fft, its leading dimension is 2 n_bins of n_fft), the
// block's cosine columns and its sine columns; they share the B operand.  B is evaluated as it is read from LDS: a sample belongs
// to taps / hop frames with another window tap (and in fbank another mean and another predecessor) in each, so it cannot be
// stored with the span.  An odd K gets one zero k, bins past n_bins are computed on a clamped column and never used.  The MFMA
// is a k-ordered chain of f32 fused multiply-adds: the bounds of features.py and fbank.py rest on that.
//
// Where the basis lives: in global memory, read as fragments through L2.  It is taps x 2 n_bins floats -- 643 KB at n_fft
// 400, 16.8 MB at 2048 -- and a workgroup uses every element of it exactly once, each by one wave: there is nothing for LDS to
// share between the waves, so streaming it through LDS would add a store, a barrier and a load to every element for no reuse.
// A fragment load is two runs of 32 neighbouring floats per wave, full 128-byte lines; per k-step a wave fetches 512 bytes
// against 128 cycles of MFMA, 16 bytes per clock per CU at full rate, a quarter of what L2 gives a CU.  At n_fft 400 the whole
// basis stays in L2 (4 MB per XCD) across the launch.  The loads of the next AHEAD k-steps are issued ahead of the MFMAs of the
// current AHEAD (a kernel's own constant: its B operand decides what registers are left for them).
//
// The epilogue stays on chip.  A wave turns its block into power (P = re^2 + im^2, both in the same lane and register; fbank:
// or its root) in LDS, [bin][frame]; after a round of eight blocks all threads add the round's bins to the mel sums,
// M[m][t] += fb[m][k] P[k][t], ascending k, f32 fused multiply-adds on the VALU (the projection is a tenth of the DFT's
// arithmetic; fb is dense, the caller's), the sums in LDS between rounds.  Then the kernel's floor and log, and the store: lane t
// of 32 stores frame t0 + t of mel m, neighbouring lanes neighbouring frames.  Every element of `out` has exactly one writer; no
// atomics; all loads and stores are plain vector ones.
//
// Contraction: alac_features.o is compiled with the compiler's default, alac_fbank.o with -ffp-contract=off, and this header
// rounds the same in both.  Every multiply-add in it is a __builtin_fmaf or the MFMA builtin; no product here feeds an addition
// that a compiler could fuse (the product inside alac_stft_mel_power is the addend of an explicit fma).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ALAC_FEATURES_THREADS = 256;
constexpr uint32_t ALAC_FEATURES_TILE = 32u;            // frames of a tile: the N of v_mfma_f32_32x32x2_f32
constexpr uint32_t ALAC_FEATURES_BLOCK = 32u;           // bins of a block: its M
constexpr uint32_t ALAC_FEATURES_ROUND_BLOCKS = 8u;     // bin blocks whose power is in LDS at a time (two per wave)
constexpr uint32_t ALAC_FEATURES_MIN_NFFT = 16u;
constexpr uint32_t ALAC_FEATURES_MAX_NFFT = 2048u;
constexpr uint32_t ALAC_FEATURES_MAX_MELS = 256u;
constexpr uint32_t ALAC_FEATURES_MAX_SPAN = 19456u;     // samples of a tile's span: 76 KiB of LDS (+ 4 KiB of skew at most)
constexpr size_t ALAC_FEATURES_LDS_DEFAULT = 64u << 10; // what a launch may ask for without an attribute
constexpr size_t ALAC_FEATURES_LDS_MAX = 160u << 10;    // what a CU has

// The frames a workgroup takes: ALAC_FEATURES_TILE, fewer only where the span of that many, (tile - 1) hop + taps samples,
// is more than ALAC_FEATURES_MAX_SPAN (hop above 561 at 2048 taps); one frame's span, taps, always fits.
__host__ __device__ inline uint32_t alac_features_tile(uint32_t taps, uint32_t hop) {
    if ((ALAC_FEATURES_TILE - 1u) * hop + taps <= ALAC_FEATURES_MAX_SPAN) return ALAC_FEATURES_TILE;
    return 1u + (ALAC_FEATURES_MAX_SPAN - taps) / hop;
}

// The span in LDS: sample i of it lives at i + skew * (i / hop).  The lanes of a wave read the same tap of 32 neighbouring
// frames, hop samples apart: with an even hop (160: every lane in one of two banks) one float of padding per hop makes the
// stride odd and the 32 addresses fall into 32 banks.
__host__ __device__ inline uint32_t alac_features_skew(uint32_t hop) { return (hop & 1u) ? 0u : 1u; }

// LDS: the window, the mel sums, the power of a round of bin blocks, what the kernel keeps of its own (`extra` floats: none
// for log-mel, the means of the tile's frames for fbank, the means and the energies for MFCC), the skewed span
struct alac_features_lds {
    uint32_t window, mel, power, extra, span;   // floats of each part, in this order
    __host__ __device__ size_t bytes() const { return sizeof(float) * ((size_t)window + mel + power + extra + span); }
};

__host__ __device__ inline alac_features_lds alac_features_lds_layout(uint32_t taps, uint32_t n_fft, uint32_t hop, uint32_t n_mels,
                                                                      uint32_t extra) {
    const uint32_t n_bins = n_fft / 2u + 1u;
    const uint32_t blocks = (n_bins + ALAC_FEATURES_BLOCK - 1u) / ALAC_FEATURES_BLOCK;
    const uint32_t span = (alac_features_tile(taps, hop) - 1u) * hop + taps;
    alac_features_lds l;
    l.window = (taps + 3u) & ~3u;
    l.mel = n_mels * ALAC_FEATURES_TILE;
    l.power = (blocks < ALAC_FEATURES_ROUND_BLOCKS ? blocks : ALAC_FEATURES_ROUND_BLOCKS) * ALAC_FEATURES_BLOCK * ALAC_FEATURES_TILE;
    l.extra = extra;
    l.span = span + alac_features_skew(hop) * ((span - 1u) / hop + 1u);
    return l;
}

// What both launches are given (alacgpu_stages.hip: launch_stft_mel fills it)
struct alac_stft_mel_params {
    const float* src;             // [planes, src_stride]
    uint64_t src_stride;
    uint64_t frames;              // the samples of a plane that are signal
    float* out;                   // [planes, n_mels, out_frames]
    uint64_t out_frames;          // >= 1
    const float* window;          // [taps]
    const float* basis;           // [taps, 2 * n_bins]
    const float* fb;              // [n_mels, n_bins]
    uint32_t taps;                // the K of the GEMM: log-mel's n_fft, fbank's win
    uint32_t n_fft, hop, n_mels;
    uint32_t tile;                // alac_features_tile(taps, hop)
    uint32_t tiles;               // ceil(out_frames / tile): blockIdx.x = plane * tiles + tile index
};

enum { ALAC_FEATURES_LOG_NONE = 0, ALAC_FEATURES_LOG_LN = 1, ALAC_FEATURES_LOG_10 = 2 };

struct alac_features_params : alac_stft_mel_params {   // frames: L > n_fft / 2; out_frames: 1 + frames / hop
    uint32_t log_mode;
    float floor;
};

__global__ void alac_logmel_kernel(alac_features_params p);

typedef float alac_f32x16 __attribute__((ext_vector_type(16)));

// P of a bin: fma(re, re, round(im * im))
__device__ __forceinline__ float alac_stft_mel_power(float re, float im) { return __builtin_fmaf(re, re, im * im); }

// A thread's view of its workgroup's tile, and the two steps of the tile body: load, then (after whatever the kernel does to
// the span of its own, behind a barrier of its own) transform.
struct alac_stft_mel_tile {
    const alac_stft_mel_params& p;
    uint32_t tid;
    uint32_t t;                   // the frame of the tile: the lane's column of B and of D
    uint32_t h;                   // the lane's k of a k-step, and its half of D's rows
    uint32_t wave;                // rotated: the wave that gets the odd block out is another SIMD's in the next workgroup
    uint32_t n_bins, skew;
    alac_features_lds lay;
    float *win, *mel, *pw, *extra, *xs;   // the parts of LDS; xs: see alac_features_skew
    uint64_t plane, t0;           // the plane and the first frame of the tile
    uint32_t nt;                  // the tile's frames
    const float* src;             // the plane's samples
    bool frame_ok;                // the lane has a frame
    uint32_t xbase;               // where the lane's frame begins in xs (tap n = q hop + r of it: xs[xbase + n + skew * q])

    __device__ __forceinline__ alac_stft_mel_tile(const alac_stft_mel_params& p_, float* lds, uint32_t extra_floats) : p(p_) {
        tid = threadIdx.x;
        t = tid & 31u;
        h = (tid >> 5) & 1u;
        wave = ((tid >> 6) + blockIdx.x) & 3u;
        n_bins = p.n_fft / 2u + 1u;
        skew = alac_features_skew(p.hop);
        lay = alac_features_lds_layout(p.taps, p.n_fft, p.hop, p.n_mels, extra_floats);
        win = lds;
        mel = win + lay.window;
        pw = mel + lay.mel;
        extra = pw + lay.power;
        xs = extra + lay.extra;
        const uint32_t tile_i = blockIdx.x % p.tiles;
        plane = blockIdx.x / p.tiles;
        t0 = (uint64_t)tile_i * p.tile;
        const uint64_t left = p.out_frames - t0;
        nt = left < p.tile ? (uint32_t)left : p.tile;
        src = p.src + plane * p.src_stride;
        frame_ok = t < nt;
        xbase = frame_ok ? t * (p.hop + skew) : 0u;
    }

    // The window, zeroed mel sums and the span into LDS, and the barrier behind them.  Frame 0 of the plane begins at sample
    // `first` (negative where frames are centred); sample(g) is the value of the span at index g of the plane, any g: the kernel
    // decides what lies outside [0, frames) and reads nothing there.
    template <typename Sample>
    __device__ __forceinline__ void load(int64_t first, Sample sample) const {
        for (uint32_t i = tid; i < p.taps; i += ALAC_FEATURES_THREADS) win[i] = p.window[i];
        for (uint32_t i = tid; i < lay.mel; i += ALAC_FEATURES_THREADS) mel[i] = 0.0f;
        const int64_t s_lo = (int64_t)(t0 * p.hop) + first;
        const uint32_t span = (p.tile - 1u) * p.hop + p.taps;
        for (uint32_t idx = tid; idx < span; idx += ALAC_FEATURES_THREADS) xs[idx + skew * (idx / p.hop)] = sample(s_lo + (int64_t)idx);
        __syncthreads();
    }

    // The rounds, which leave the finished mel sums in LDS (mel[m * ALAC_FEATURES_TILE + t], behind a barrier; thread (m, t)
    // wrote the sum it owns).  tap(n, q, r): the B operand of tap n = q hop + r of the lane's frame (called for lanes with a
    // frame and n < taps only); power(re, im): what a bin adds to the mel sums.
    template <uint32_t AHEAD, typename Tap, typename Power>
    __device__ __forceinline__ void rounds(Tap tap, Power power) const {
        const uint32_t taps = p.taps, hop = p.hop, n_mels = p.n_mels;
        const uint32_t ldb = 2u * n_bins;
        const uint32_t n_blocks = (n_bins + ALAC_FEATURES_BLOCK - 1u) / ALAC_FEATURES_BLOCK;
        const uint32_t pairs = taps / 2u;         // k-steps with both taps inside

        for (uint32_t round0 = 0; round0 < n_blocks; round0 += ALAC_FEATURES_ROUND_BLOCKS) {
            const uint32_t round_end = round0 + ALAC_FEATURES_ROUND_BLOCKS < n_blocks ? round0 + ALAC_FEATURES_ROUND_BLOCKS : n_blocks;
            for (uint32_t blk = round0 + wave; blk < round_end; blk += 4u) {
                uint32_t col = blk * ALAC_FEATURES_BLOCK + t;     // (t: the lane's row of A as well)
                col = col < n_bins ? col : n_bins - 1u;
                const float* a_re = p.basis + col + (size_t)h * ldb;
                const float* a_im = a_re + n_bins;
                const size_t a_step = 2u * (size_t)ldb;
                alac_f32x16 re = {}, im = {};
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
                // what is left: up to AHEAD - 1 whole k-steps and, for an odd K, one with the tap of h = 1 outside
                for (; 2u * s < taps; ++s) {
                    const bool ok = n < taps;
                    const float vr = ok ? a_re[0] : 0.0f;
                    const float vi = ok ? a_im[0] : 0.0f;
                    const float b = (ok && frame_ok) ? tap(n, q, r) : 0.0f;
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(vr, b, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(vi, b, im, 0, 0, 0);
                    if (2u * s + 2u < taps) {      // (the next step exists: its row h = 0 is inside the basis)
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
                    dst[row * ALAC_FEATURES_TILE] = power(re[j], im[j]);
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
    }

    // The store: finish(v) is what is stored for a mel sum v (a thread reads the sums it wrote itself)
    template <typename Finish>
    __device__ __forceinline__ void store(Finish finish) const {
        const uint32_t n_mels = p.n_mels;
        if (frame_ok) {
            float* const out = p.out + plane * n_mels * p.out_frames + t0 + t;
            for (uint32_t m = tid >> 5; m < n_mels; m += ALAC_FEATURES_THREADS / 32u)
                out[(uint64_t)m * p.out_frames] = finish(mel[m * ALAC_FEATURES_TILE + t]);
        }
    }

    // What the log-mel and the fbank kernel do: the rounds, then the store
    template <uint32_t AHEAD, typename Tap, typename Power, typename Finish>
    __device__ __forceinline__ void transform(Tap tap, Power power, Finish finish) const {
        rounds<AHEAD>(tap, power);
        store(finish);
    }
};
