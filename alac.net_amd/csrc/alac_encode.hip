// alac_encode.hip -- the ALAC encoder on gfx950: PCM from an int32 / float32 tensor to ALAC packets, one wave per packet.
//
// Fixed policy (what every packet is made of):
//   * 16-bit: no uncompressed low bytes (ub = 0).  24-bit: ub = 1, mono and stereo alike: the low byte of every sample goes
//     into the packet as is and the predictor sees sample >> 8.  The reference rebuilds both (AlacFile.cs:549-553 mono,
//     :381-388 stereo); its 16-bit output paths ignore the low bytes (:531-540, Deinterlace16), so 16-bit never uses them.
//   * stereo: mix_shift 2 with mix_weight 0..4 -- seven channel streams (L, R; A_w = R + ((L - R) * w >> 2) for w = 1..4;
//     B = L - R), the smallest pair wins, a tie goes to the smaller weight.  Mono: one stream.
//   * per channel: predictionType 0, LPC order 8 quantised at q = 9 (Levinson-Durbin in double on the autocorrelation over
//     lags 0..8; A_w's from L's and R's auto- and cross-correlation), ricemodifier 4; pb / mb / kb from the stream cfg.
//   * an escape packet (raw samples) whenever the compressed packet would not be smaller, or the decoder's state machine
//     cannot express it (a zero run under a kb that is a multiple of 32); so no packet is larger than
//     alacgpu_encode_max_packet_bytes.
//   * hassize exactly when the packet is shorter than max_samples_per_frame; END tag, then zeros to the byte.
// The forward predictor and the Rice coder run the decoder's state machines (AlacFile.cs:256-336 coefficient adaptation,
// :214-252 history, k and zero runs); the packet is the one synth/alac_synth.c writes for the same recipe, bit for bit.
//
// Work of one packet, in three launches (one wave per packet each): every lane sums part of the autocorrelation, lanes 0..6
// run the seven candidate chains (predictor and Rice history, lengths only) side by side, and the choice is made
// (analyse); lanes 0 and 1 run the chosen pair again and store each frame's code (codes); a scan of the code lengths gives
// every field its bit position, and each lane assembles a range of output words from the fields that overlap it (emit).
// The PCM is read in chunks of CH frames staged in LDS; the codes and positions live in a per-workgroup workspace of the
// context.  (One kernel doing all three needed more SGPRs than a wave has and spilled them into VGPR lanes.)
#include "alac_encode.h"
#include "alacgpu.h"

namespace {

constexpr int CH = 512;           // frames per LDS chunk
constexpr int HALO = 8;           // frames in front of a chunk the autocorrelation needs
constexpr int NS = 7;             // candidate streams of a two-channel packet
constexpr int ORDER = 8, QUANT = 9, RICEMOD = 4, MIX_SHIFT = 2;
constexpr int LAGS = ORDER + 1;
constexpr uint32_t HDR = ALAC_ENC_HDR_ITEMS;

__device__ __forceinline__ int32_t w_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int32_t w_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
__device__ __forceinline__ int32_t w_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
__device__ __forceinline__ int32_t sx(int32_t v, int rss) { const int m = 32 - rss; return (int32_t)((uint32_t)v << m) >> m; }
__device__ __forceinline__ int clz_q(int32_t x) { return x == 0 ? 40 : __clz(x); }   // AlacFile.cs:170-191: 40 for 0

// frame `frame`, channel c of the source as the canonical sample: int32 clamped to the sample range, float32
// round(x * 2^(ss-1)) clamped (NaN: the smallest sample)
__device__ __forceinline__ int32_t load_sample(const alac_encode_params& p, uint64_t frame, uint32_t c, int ss) {
    const uint64_t idx = p.layout == ALACGPU_DST_PLANAR ? (uint64_t)c * p.plane_stride + frame : frame * p.channels + c;
    const int32_t hi = (1 << (ss - 1)) - 1, lo = -hi - 1;
    if (p.dtype == ALACGPU_DST_FLOAT32) {
        const float y = fminf(fmaxf(((const float*)p.pcm)[idx] * (float)(1 << (ss - 1)), (float)lo), (float)hi);
        return (int32_t)rintf(y);
    }
    const int32_t v = ((const int32_t*)p.pcm)[idx];
    return v < lo ? lo : (v > hi ? hi : v);
}

// channel stream s of a frame (after the low bytes are split off): 0 L, 1 R, 2..5 A_w (w = s - 1), 6 B = L - R
__device__ __forceinline__ int32_t stream_value(int s, int32_t l, int32_t r) {
    if (s == 0) return l;
    if (s == 1) return r;
    if (s == NS - 1) return w_sub(l, r);
    return w_add(r, w_mul(w_sub(l, r), s - 1) >> MIX_SHIFT);   // inverse of AlacFile.cs:349-350
}

// one adaptive Golomb-Rice symbol (the inverse of EntropyDecodeValue, AlacFile.cs:193-212), appended to (code, len);
// written with selects, not branches (the chains run on a few lanes of the wave)
__device__ __forceinline__ void put_symbol(uint32_t v, int k, uint32_t m, int esc_bits, uint64_t& code, uint32_t& len) {
    m = m == 0 ? 1u : m;   // (only in a chain already marked unusable)
    const uint32_t x = v / m, rem = v - x * m;
    const bool raw = x > 8;   // nine ones, then the raw value
    const uint32_t xu = raw ? 0u : x;
    // x ones and a zero, then nothing (k = 1), k - 1 zeros (the decoder reads k bits, sees <= 1 and un-reads one) or rem + 1
    const uint32_t tl = k == 1 ? 0u : (rem == 0 ? (uint32_t)k - 1u : (uint32_t)k);
    const uint64_t tv = (k == 1 || rem == 0) ? 0ull : (uint64_t)(rem + 1u);
    const uint64_t cn = ((((1ull << xu) - 1ull) << 1) << tl) | tv;
    const uint64_t cr = (0x1FFull << esc_bits) | (uint64_t)(v & ((1u << esc_bits) - 1u));
    const uint32_t l = raw ? 9u + (uint32_t)esc_bits : xu + 1u + tl;
    code = (code << l) | (raw ? cr : cn);
    len += l;
}

struct RiceCfg {
    int rss, kmod;
    uint32_t kmask;
    int32_t hist_mult;
};

// One channel stream through the forward adaptive predictor (inverse of PredictorDecompressFirAdapt, AlacFile.cs:256-336)
// and the Rice coder (mirror of EntropyRiceDecode, AlacFile.cs:214-252), one frame per step.  EMIT: frame i's code -- its
// symbol and, when a zero run follows it, the run's count -- goes to item i (frames inside a run get empty items).
struct Chain {
    int32_t x[LAGS];       // x[0] = out[i-9] .. x[8] = out[i-1]
    int32_t coef[ORDER];
    int32_t history;
    uint32_t signmod;
    bool counting, ok;
    uint32_t z, m2, pend_len, pend_idx;
    int k2;
    uint64_t pend_code, bits;

    __device__ __forceinline__ void init(const int32_t* c, int32_t init_hist) {
#pragma unroll
        for (int j = 0; j < LAGS; j++) x[j] = 0;
#pragma unroll
        for (int j = 0; j < ORDER; j++) coef[j] = c[j];
        history = init_hist;
        signmod = 0;
        counting = false;
        ok = true;
        z = m2 = pend_len = pend_idx = 0;
        k2 = 0;
        pend_code = 0;
        bits = 0;
    }

    template <bool EMIT>
    __device__ __forceinline__ void item(uint32_t i, uint64_t code, uint32_t len, uint64_t* ic, uint32_t* il) {
        bits += len;
        if (EMIT) { ic[i] = code; il[i] = len; }
    }

    template <bool EMIT>
    __device__ __forceinline__ void end_run(uint64_t* ic, uint32_t* il) {
        put_symbol(z, k2, m2, 16, pend_code, pend_len);
        item<EMIT>(pend_idx, pend_code, pend_len, ic, il);
        counting = false;
    }

    template <bool EMIT>
    __device__ __forceinline__ void step(uint32_t i, int32_t v, uint32_t n, const RiceCfg& rc, uint64_t* ic, uint32_t* il) {
        // :297-334 (frames 0 .. 8 are the warm-up, :284-293: the first as is, then first differences)
        const int32_t b0 = x[0];
        int32_t sum = 0;
#pragma unroll
        for (int j = 0; j < ORDER; j++) sum = w_add(sum, w_mul(w_sub(x[ORDER - j], b0), coef[j]));
        const int32_t pred = w_add(w_add((int32_t)(1 << (QUANT - 1)), sum) >> QUANT, b0);
        const int32_t e = i == 0 ? v : sx(w_sub(v, i <= (uint32_t)ORDER ? x[LAGS - 1] : pred), rc.rss);
        {   // identical adaptation, :312-332, as selects
            const bool positive = e > 0;
            int32_t ee = e;
            bool go = i > (uint32_t)ORDER;
#pragma unroll
            for (int q = ORDER - 1; q >= 0; q--) {
                go = go && (positive ? ee > 0 : ee < 0);
                int32_t val = w_sub(b0, x[ORDER - q]);
                const int32_t sg = val < 0 ? -1 : (val > 0 ? 1 : 0);
                const int32_t sign = go ? (positive ? sg : -sg) : 0;
                coef[q] = w_sub(coef[q], sign);
                val = w_mul(val, sign);
                ee = w_sub(ee, w_mul(val >> QUANT, ORDER - q));
            }
        }
#pragma unroll
        for (int j = 0; j < LAGS - 1; j++) x[j] = x[j + 1];
        x[LAGS - 1] = v;

        const uint32_t dv = e >= 0 ? (uint32_t)e * 2u : (uint32_t)(-(int64_t)e) * 2u - 1u;   // inverse of :225-226
        if (counting) {
            if (dv == 0) {   // one more frame of the zero run
                z++;
                item<EMIT>(i, 0, 0, ic, il);
                if (i + 1 == n) end_run<EMIT>(ic, il);
                return;
            }
            end_run<EMIT>(ic, il);
            history = 0;
            signmod = 1;
        }
        const int kk = 31 - clz_q(w_add(history >> 9, 3));
        const int k = kk < rc.kmod ? kk : rc.kmod;   // :221-222
        if (k < 1) ok = false;
        const int kq = k < 1 ? 1 : k;
        uint64_t code = 0;
        uint32_t len = 0;
        put_symbol(dv - signmod, kq, (1u << kq) - 1u, rc.rss, code, len);
        signmod = 0;
        history = dv > 0xFFFFu ? 0xFFFF
                               : w_sub(w_add(history, w_mul((int32_t)dv, rc.hist_mult)), w_mul(history, rc.hist_mult) >> 9);   // :229
        if (history < 128 && i + 1 < n) {   // a zero-run count follows this symbol (:231-249)
            k2 = clz_q(history) + ((history + 16) / 64) - 24;
            m2 = ((1u << (k2 & 31)) - 1u) & rc.kmask;
            if (m2 == 0 || k2 < 1) ok = false;
            counting = true;
            z = 0;
            pend_code = code;
            pend_len = len;
            pend_idx = i;
        } else {
            item<EMIT>(i, code, len, ic, il);
        }
    }
};

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Packet {
    uint32_t n;
    uint64_t first;
    int ss, stereo, ub, hassize;
    RiceCfg rc;
    int32_t init_hist;
};

// stage frames c0 - HALO .. c0 + cn - 1 (the low bytes split off) into sh_l / sh_r
__device__ __forceinline__ void stage(const alac_encode_params& p, const Packet& k, uint32_t c0, uint32_t cn, int32_t* sh_l,
                                      int32_t* sh_r) {
    for (uint32_t t = threadIdx.x; t < cn + HALO; t += ALAC_ENC_THREADS) {
        const int64_t f = (int64_t)c0 + t - HALO;
        int32_t l = 0, r = 0;
        if (f >= 0) {
            l = load_sample(p, k.first + (uint64_t)f, 0, k.ss) >> (8 * k.ub);   // arithmetic (AlacFile.cs:383-388)
            if (k.stereo) r = load_sample(p, k.first + (uint64_t)f, 1, k.ss) >> (8 * k.ub);
        }
        sh_l[t] = l;
        sh_r[t] = r;
    }
}

// the chains of `lanes` lanes over the whole packet: lane j runs stream sid with coefficients coefs
template <bool EMIT>
__device__ __forceinline__ Chain run_chains(const alac_encode_params& p, const Packet& k, int lanes, int sid, const int32_t* coefs,
                                            uint64_t* ic, uint32_t* il, int32_t* sh_l, int32_t* sh_r) {
    Chain ch;
    const bool mine = (int)threadIdx.x < lanes;
    ch.init(coefs, k.init_hist);
    for (uint32_t c0 = 0; c0 < k.n; c0 += CH) {
        const uint32_t cn = min((uint32_t)CH, k.n - c0);
        stage(p, k, c0, cn, sh_l, sh_r);
        __syncthreads();
        if (mine)
            for (uint32_t t = 0; t < cn; t++)
                ch.step<EMIT>(c0 + t, stream_value(sid, sh_l[t + HALO], sh_r[t + HALO]), k.n, k.rc, ic, il);
        __syncthreads();
    }
    return ch;
}

// The packet's facts from the tables and its stream cfg; returns its status (ALACGPU_ST_OK_D: encode it).
__device__ __forceinline__ int packet_facts(const alac_encode_params& p, uint32_t pk, Packet& k, alacgpu_cfg_dev& cfg) {
    const uint32_t ci = p.cfg_idx[pk];
    int st = ALACGPU_ST_OK_D;
    cfg = alacgpu_cfg_dev{};
    if (ci >= p.n_cfgs) st = ALACGPU_ST_UNSUPPORTED_PARAMS_D;
    else cfg = p.cfgs[ci];
    k.n = p.src_frames[pk];
    k.first = p.src_first[pk];
    k.ss = cfg.sample_size;
    if (!st && k.ss != 16 && k.ss != 24) st = ALACGPU_ST_UNSUPPORTED_SAMPLE_SIZE_D;
    if (!st && (k.n == 0 || k.n > min(cfg.max_samples_per_frame, 16384u))) st = ALACGPU_ST_BAD_SAMPLE_COUNT_D;
    if (!st) {   // the run lies inside the source
        const uint64_t lead = p.layout == ALACGPU_DST_PLANAR ? (uint64_t)(p.channels - 1u) * p.plane_stride : 0u;
        const uint64_t cap = p.layout == ALACGPU_DST_PLANAR ? (lead <= p.src_elems ? p.src_elems - lead : 0u)
                                                            : p.src_elems / p.channels;
        if (lead > p.src_elems || k.first > cap || k.n > cap - k.first) st = ALACGPU_ST_DEST_RANGE_D;
    }
    k.stereo = p.channels == 2;
    k.ub = k.ss == 24 ? 1 : 0;
    k.hassize = k.n != cfg.max_samples_per_frame;
    k.rc.rss = k.ss - 8 * k.ub + k.stereo;
    k.rc.kmod = cfg.rice_kmodifier;
    k.rc.kmask = (1u << (cfg.rice_kmodifier & 31)) - 1u;
    k.rc.hist_mult = RICEMOD * (cfg.rice_history_mult / 4);   // :483, :643
    k.init_hist = cfg.rice_initial_history;
    return st;
}

// the candidate streams of the chosen mix weight w: channel A's and channel B's
__device__ __forceinline__ int stream_a(const Packet& k, int w) { return !k.stereo ? 0 : (w == 0 ? 0 : 1 + w); }
__device__ __forceinline__ int stream_b(int w) { return w == 0 ? 1 : NS - 1; }

}  // namespace

// Pass 1: status, LPC of every candidate stream, the candidates' code lengths, the choice; writes the header fields
// (items 0 .. 20: escape flag, mix weight and the chosen streams' coefficients are read back from there by pass 2).
__global__ __launch_bounds__(ALAC_ENC_THREADS) void alac_encode_analyse_kernel(alac_encode_params p) {
    __shared__ int32_t sh_l[CH + HALO], sh_r[CH + HALO];
    __shared__ int32_t sh_coef[NS][ORDER];
    __shared__ uint64_t sh_bits[NS];
    __shared__ int sh_ok[NS];
    __shared__ int sh_esc, sh_w;
    const int lane = threadIdx.x;
    const uint32_t pk = p.first_packet + blockIdx.x;
    if (pk >= p.n_packets) return;
    uint64_t* code = p.ws_code + (uint64_t)blockIdx.x * alac_enc_items(p.smax);
    uint32_t* pos = p.ws_pos + (uint64_t)blockIdx.x * (alac_enc_items(p.smax) + 1);
    Packet k;
    alacgpu_cfg_dev cfg;
    const int st = packet_facts(p, pk, k, cfg);
    if (st) {
        if (lane == 0) { p.status[pk] = st; p.sizes[pk] = 0; }
        return;
    }
    const int nch = k.stereo ? 2 : 1;
    const int nstreams = k.stereo ? NS : 1;
    // ---- autocorrelation: L's and R's own and cross sums over lags 0..8 ---------------------------------------------
    double all[LAGS], arr[LAGS], alr[LAGS], arl[LAGS];   // sum l[i] l[i-j], r r, l[i] r[i-j], r[i] l[i-j]
#pragma unroll
    for (int j = 0; j < LAGS; j++) all[j] = arr[j] = alr[j] = arl[j] = 0.0;
    for (uint32_t c0 = 0; c0 < k.n; c0 += CH) {
        const uint32_t cn = min((uint32_t)CH, k.n - c0);
        stage(p, k, c0, cn, sh_l, sh_r);
        __syncthreads();
        for (uint32_t t = lane; t < cn; t += ALAC_ENC_THREADS) {
            const double l = sh_l[t + HALO], r = sh_r[t + HALO];
#pragma unroll
            for (int j = 0; j < LAGS; j++) {   // (frames in front of the packet are staged as 0)
                const double lj = sh_l[t + HALO - j], rj = sh_r[t + HALO - j];
                all[j] += l * lj;
                arr[j] += r * rj;
                alr[j] += l * rj;
                arl[j] += r * lj;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < LAGS; j++) {
        all[j] = wave_sum(all[j]);
        arr[j] = wave_sum(arr[j]);
        alr[j] = wave_sum(alr[j]);
        arl[j] = wave_sum(arl[j]);
    }

    // ---- LPC of every candidate stream: Levinson-Durbin at order 8, quantised at q = 9 -----------------------------
    if (lane < nstreams) {
        // stream = a L + b R (A_w up to its rounding, which the choice of coefficients may ignore)
        const double a = lane == 0 ? 1.0 : lane == 1 ? 0.0 : lane == NS - 1 ? 1.0 : 0.25 * (lane - 1);
        const double b = lane == 0 ? 0.0 : lane == 1 ? 1.0 : lane == NS - 1 ? -1.0 : 1.0 - a;
        double r[LAGS], c[LAGS], tmp[LAGS];
#pragma unroll
        for (int j = 0; j < LAGS; j++) {
            r[j] = a * a * all[j] + b * b * arr[j] + a * b * (alr[j] + arl[j]);
            c[j] = 0.0;
        }
        bool live = k.n > (uint32_t)(ORDER + 1) && r[0] > 0.0;
        r[0] *= 1.0 + 1e-9;
        double err = r[0];
#pragma unroll
        for (int i = 1; i <= ORDER; i++) {
            if (live) {
                double acc = r[i];
#pragma unroll
                for (int j = 1; j < i; j++) acc -= c[j] * r[i - j];
                const double kk = acc / err;
#pragma unroll
                for (int j = 0; j < LAGS; j++) tmp[j] = c[j];
                c[i] = kk;
#pragma unroll
                for (int j = 1; j < i; j++) c[j] = tmp[j] - kk * tmp[i - j];
                err *= 1.0 - kk * kk;
                if (!(err > 0.0)) live = false;
            }
        }
        const bool any = k.n > (uint32_t)(ORDER + 1) && r[0] > 0.0;
#pragma unroll
        for (int j = 0; j < ORDER; j++) {
            double q = floor(c[j + 1] * (double)(1 << QUANT) + 0.5);
            q = q > 32767.0 ? 32767.0 : (q < -32768.0 ? -32768.0 : q);
            sh_coef[lane][j] = any ? (int32_t)q : 0;
        }
    }
    __syncthreads();

    // ---- the candidates: code lengths of every stream -----------------------------------------------------------------
    {
        const int sid = lane < nstreams ? lane : 0;
        const Chain cand = run_chains<false>(p, k, nstreams, sid, sh_coef[sid], nullptr, nullptr, sh_l, sh_r);
        if (lane < nstreams) {
            sh_bits[lane] = cand.bits;
            sh_ok[lane] = cand.ok;
        }
    }
    __syncthreads();
    if (lane == 0) {
        uint64_t best = ~0ull;
        int w = 0;
        if (!k.stereo) {
            if (sh_ok[0]) best = sh_bits[0];
        } else {
            for (int cw = 0; cw <= 4; cw++) {
                const int sa = cw == 0 ? 0 : 1 + cw, sb = cw == 0 ? 1 : NS - 1;
                if (sh_ok[sa] && sh_ok[sb] && sh_bits[sa] + sh_bits[sb] < best) { best = sh_bits[sa] + sh_bits[sb]; w = cw; }
            }
        }
        const uint64_t hdr = 23 + 32 * k.hassize + 16 + nch * (16 + 16 * ORDER);
        const uint64_t esc_bits = 23 + 32 * k.hassize + (uint64_t)k.n * nch * k.ss + 3;
        const uint64_t comp_bits = best == ~0ull ? ~0ull : hdr + (uint64_t)k.n * nch * 8 * k.ub + best + 3;
        sh_esc = comp_bits == ~0ull || (comp_bits + 7) / 8 >= (esc_bits + 7) / 8;
        sh_w = w;
    }
    __syncthreads();
    const int esc = sh_esc, w = sh_w;
    if (lane == 0) {
        const int ub = esc ? 0 : k.ub;
        const uint32_t n = k.n;
        code[0] = ((uint64_t)(k.stereo ? 1 : 0) << 20) | ((uint64_t)k.hassize << 3) | ((uint64_t)ub << 1) | (uint64_t)esc;
        pos[0] = 23;
        code[1] = n;
        pos[1] = k.hassize ? 32 : 0;
        code[2] = k.stereo ? ((uint64_t)MIX_SHIFT << 8) | (uint64_t)w : 0;
        pos[2] = esc ? 0 : 16;
        for (int c = 0; c < 2; c++) {
            const bool on = !esc && c < nch;
            const int s = c == 0 ? stream_a(k, w) : stream_b(w);
            code[3 + 9 * c] = (uint64_t)((QUANT << 8) | (RICEMOD << 5) | ORDER);   // predictionType 0
            pos[3 + 9 * c] = on ? 16 : 0;
            for (int j = 0; j < ORDER; j++) {
                code[4 + 9 * c + j] = (uint64_t)((uint32_t)sh_coef[s][j] & 0xFFFFu);
                pos[4 + 9 * c + j] = on ? 16 : 0;
            }
        }
        code[HDR + 3 * n] = 7;   // END element tag
        pos[HDR + 3 * n] = 3;
        p.status[pk] = ALACGPU_ST_OK_D;
    }
}

// Pass 2: every frame's fields -- low bytes or raw samples, then channel A's and channel B's codes from the chosen chains.
__global__ __launch_bounds__(ALAC_ENC_THREADS) void alac_encode_codes_kernel(alac_encode_params p) {
    __shared__ int32_t sh_l[CH + HALO], sh_r[CH + HALO];
    __shared__ int32_t sh_coef[2][ORDER];
    const int lane = threadIdx.x;
    const uint32_t pk = p.first_packet + blockIdx.x;
    if (pk >= p.n_packets || p.status[pk] != ALACGPU_ST_OK_D) return;
    uint64_t* code = p.ws_code + (uint64_t)blockIdx.x * alac_enc_items(p.smax);
    uint32_t* pos = p.ws_pos + (uint64_t)blockIdx.x * (alac_enc_items(p.smax) + 1);
    Packet k;
    alacgpu_cfg_dev cfg;
    (void)packet_facts(p, pk, k, cfg);
    const int nch = k.stereo ? 2 : 1;
    const int esc = (int)(code[0] & 1u), ub = (int)((code[0] >> 1) & 3u), w = (int)(code[2] & 0xFFu);
    if (lane < 2 * ORDER) sh_coef[lane / ORDER][lane % ORDER] = (int32_t)(int16_t)(uint16_t)code[4 + 9 * (lane / ORDER) + lane % ORDER];
    __syncthreads();
    const uint32_t n = k.n;
    uint64_t* c_frm = code + HDR;
    uint32_t* l_frm = pos + HDR;
    uint64_t* c_a = code + HDR + n;
    uint32_t* l_a = pos + HDR + n;
    uint64_t* c_b = code + HDR + 2 * n;
    uint32_t* l_b = pos + HDR + 2 * n;
    for (uint32_t i = lane; i < n; i += ALAC_ENC_THREADS) {
        uint64_t fc = 0;
        uint32_t fl = 0;
        if (esc || ub) {
            const int32_t l = load_sample(p, k.first + i, 0, k.ss);
            const int32_t r = k.stereo ? load_sample(p, k.first + i, 1, k.ss) : 0;
            const int bits = esc ? k.ss : 8 * ub;
            const uint64_t m = (1ull << bits) - 1ull;
            fc = k.stereo ? (((uint64_t)(uint32_t)l & m) << bits) | ((uint64_t)(uint32_t)r & m) : ((uint64_t)(uint32_t)l & m);
            fl = bits * nch;
        }
        c_frm[i] = fc;
        l_frm[i] = fl;
        if (esc) { c_a[i] = 0; l_a[i] = 0; }
        if (esc || !k.stereo) { c_b[i] = 0; l_b[i] = 0; }
    }
    if (!esc) {
        const int sid = lane == 1 ? stream_b(w) : stream_a(k, w);
        run_chains<true>(p, k, nch, sid, sh_coef[lane == 1 ? 1 : 0], lane == 1 ? c_b : c_a, lane == 1 ? l_b : l_a, sh_l, sh_r);
    }
}

// Pass 3: the bit position of every field (an exclusive scan of the lengths, in place), then the bytes: each lane
// assembles a contiguous range of 32-bit words from the fields that overlap it.
__global__ __launch_bounds__(ALAC_ENC_THREADS) void alac_encode_emit_kernel(alac_encode_params p) {
    const int lane = threadIdx.x;
    const uint32_t pk = p.first_packet + blockIdx.x;
    if (pk >= p.n_packets || p.status[pk] != ALACGPU_ST_OK_D) return;
    const uint64_t* code = p.ws_code + (uint64_t)blockIdx.x * alac_enc_items(p.smax);
    uint32_t* pos = p.ws_pos + (uint64_t)blockIdx.x * (alac_enc_items(p.smax) + 1);
    const uint32_t K_p = HDR + 3 * p.src_frames[pk] + 1;
    const uint32_t seg = (K_p + ALAC_ENC_THREADS - 1) / ALAC_ENC_THREADS;
    const uint32_t s0 = min((uint32_t)lane * seg, K_p), s1 = min(s0 + seg, K_p);
    uint32_t mine = 0;
    for (uint32_t i = s0; i < s1; i++) mine += pos[i];
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < ALAC_ENC_THREADS; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const uint32_t total = __shfl(incl, ALAC_ENC_THREADS - 1, 64);
    uint32_t run = incl - mine;
    for (uint32_t i = s0; i < s1; i++) {
        const uint32_t len = pos[i];
        pos[i] = run;
        run += len;
    }
    if (lane == 0) pos[K_p] = total;
    __syncthreads();

    // ---- the bytes: each lane assembles a contiguous range of 32-bit words from the fields that overlap it --------------
    const uint32_t words = (total + 31) / 32;
    const uint32_t w0 = (uint32_t)((uint64_t)words * lane / ALAC_ENC_THREADS);
    const uint32_t w1 = (uint32_t)((uint64_t)words * (lane + 1) / ALAC_ENC_THREADS);
    uint32_t* out = (uint32_t*)(p.packets + (uint64_t)pk * p.slot_bytes);
    if (w0 < w1) {
        uint32_t lo = 0, hi = K_p;   // the last field that starts at or before the range's first bit
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) / 2;
            if (pos[mid] <= w0 * 32u) lo = mid;
            else hi = mid - 1;
        }
        uint32_t f = lo;
        for (uint32_t wd = w0; wd < w1; wd++) {
            const uint32_t we = wd * 32u + 32u;
            uint32_t word = 0;
            while (f < K_p) {
                const uint32_t b0 = pos[f], b1 = pos[f + 1];
                if (b0 >= we) break;
                if (b1 > b0) {
                    const int e = (int)we - (int)b1;
                    const uint64_t cf = code[f];
                    word |= (uint32_t)(e >= 0 ? cf << e : cf >> (-e));
                }
                if (b1 <= we) f++;
                else break;
            }
            if ((uint64_t)wd * 4u + 4u <= p.slot_bytes) out[wd] = __builtin_bswap32(word);   // MSB first
        }
    }
    if (lane == 0) p.sizes[pk] = (total + 7) / 8;
}
