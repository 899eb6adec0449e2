// alacgpu_ctx.h -- what the host side's two translation units share (private: not installed): the ctx, the argument check every
// entry point opens with and the scratch protocol.  alacgpu_api.hip is the decode path, alacgpu_stages.hip the stages around it.
#ifndef ALACGPU_CTX_H
#define ALACGPU_CTX_H

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "alac_kernels.h"
#include "alacgpu.h"

constexpr int N_SLOTS = 8;          // launch pairs that may be in flight at once on one ctx (any streams)
constexpr uint32_t AB_SMALL_MAX_PACKETS = 4096;  // up to here: the build with 16-step speculative units (latency-bound launches)
constexpr uint32_t PAIR_DENSE_MIN_PACKETS = 2049;   // from here: the paired kernel's 8-packet form (more than one 4-packet workgroup per SIMD set)
constexpr uint32_t AB5_MIN_PACKETS = 10241;    // above: the 96-register build of the 8-packet arrangement (five workgroups per CU)
constexpr uint32_t DENSE_MIN_PACKETS = 12289;   // measured cross-over of the two arrangements of the main kernel
// Pairing (the paired kernel in front of the small-batch launch).  The table: a power of two of entries, at
// least PAIR_TABLE_FACTOR times the largest batch seen, in sets of PAIR_WAYS.  (A packet evicted by another sends its whole group
// of 8 through the two-pass kernel, and ONE such group makes the launch as long as both kernels: direct-mapped at 4 entries per
// packet, an eighth of cfg2's packets lost their entry and the warm call took 1.14 ms instead of 0.66.)  The verdict: the
// context looks at the counters every PAIR_WINDOW paired launches and stops the paired launch when the window saw
//   - no workgroup of the paired kernel finish (batches of one-channel packets, of orders above 8 or more than 23 bits, packets
//     that are new in every call, a working set that outgrows the table: such calls only pay the empty launch), or
//   - more packets with a wrong remembered start than packets finished (a caller that rewrites its packets in place), or
//   - from the second window on (the first holds the cold calls) more than one workgroup that left its packets per
//     PAIR_DONE_PER_LEFT groups of 4 packets that finished (the 4-packet kernel counts one per workgroup, the 8-packet kernel
//     two: a lost entry weighs the same in both): a call in which any group falls back takes as long as both kernels.
// PAIR_RETRY launches later the context tries a window again: what it decodes may have changed.
constexpr uint32_t PAIR_TABLE_FACTOR = 64, PAIR_TABLE_MIN = 1024;
constexpr unsigned PAIR_WINDOW = 16, PAIR_RETRY = 4096;
constexpr unsigned long long PAIR_DONE_PER_LEFT = 1024;
constexpr int N_HOST_STREAMS = 4;   // chunks of the host-buffer pipeline (H2D k+1 || decode k || D2H k-1)
constexpr uint32_t MAX_FRAME = 16384;   // the longest frame the reference decodes (its scratch, AlacFile.cs:28)

// ALACGPU_DENSE (A/B and tests): which build of the first launch runs.  Auto picks by batch size; "eight" picks among the
// builds of the 8-packet arrangement by batch size; the others force one build whatever the batch size.
enum dense_mode { DENSE_AUTO = -1, DENSE_EIGHT = 0, DENSE_ALWAYS = 1, DENSE_FORCE_AB5 = 2, DENSE_FORCE_SMALL = 3, DENSE_FORCE_AB = 4 };

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);              \
            return ALACGPU_ERR_HIP;                                                             \
        }                                                                                       \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A pointer argument as include/alacgpu.h describes it: the alignment it needs (a power of two) and whether it may be NULL.
// An entry point states its pointers as one list in the header's order; args_ok is false for a NULL that is required and
// for a misaligned pointer.
struct arg { const void* p; unsigned align; bool required = true; };
inline bool args_ok(std::initializer_list<arg> args) {
    for (const arg& a : args)
        if ((!a.p && a.required) || ((uintptr_t)a.p & (a.align - 1u)) != 0) return false;
    return true;
}

// What one launch pair (alac_decode_ab_kernel + alac_decode_ab32_kernel) owns while it is in flight: the group flags the
// first kernel hands to the second, and the events that bracket the pair.  A slot is reused only after its last launch
// has finished (hipEventSynchronize), so calls on different streams never share flags.
struct launch_slot {
    uint32_t* d_flags = nullptr;
    size_t flags_bytes = 0;
    int32_t* d_park = nullptr;     // destination mode: where channel A waits (n_packets * park_stride ints, grown on demand)
    size_t park_bytes = 0;
    uint64_t* d_first = nullptr;   // window calls: dst_first as alac_window_first_kernel leaves it (n_packets, grown on demand)
    size_t first_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool used = false;
};

// Device scratch the calls of a ctx share one after the other, whatever their streams: one or two grow-only buffers and the
// event behind the last call that used them.  acquire: a call that needs more than there is waits on the host for that event
// and grows; any other lets its stream wait for it.  release, behind the call's last launch, records the event on its stream.
// A call that needs none (0 bytes) does neither, so it cannot replace the event of one that does: the next still waits for that.
struct scratch {
    void* buf[2] = {};
    size_t bytes[2] = {};
    hipEvent_t done = nullptr;
    bool used = false;       // `done` has been recorded
    bool held = false;       // between an acquire of more than 0 bytes and its release
    int acquire(alacgpu_ctx* ctx, hipStream_t stream, size_t need0, size_t alloc0, size_t need1 = 0, size_t alloc1 = 0);
    int release(alacgpu_ctx* ctx, hipStream_t stream);
    void destroy();          // waits for the last user
};

struct alacgpu_ctx {
    int device = 0;
    uint32_t n_cfgs = 0;
    alacgpu_cfg* h_cfgs = nullptr;
    alacgpu_cfg_dev* d_cfgs = nullptr;
    hipStream_t streams[N_HOST_STREAMS] = {};   // used by the host-buffer entry points: range k decodes (and downloads) on streams[k]
    hipStream_t up_stream = nullptr;            // ... and every upload runs on this one, range after range
    hipEvent_t ev_up[N_HOST_STREAMS] = {};   // range k's packets (and, for k = 0, the batch's metadata) are in HBM
    launch_slot slots[N_SLOTS];
    unsigned next_slot = 0;
    int last_slot = -1;
    uint32_t out_format = 0;           // 0 int32 per sample, 1 packed little-endian PCM
    int host_chunks = 0;               // 0 auto; 1..N_HOST_STREAMS forced (ALACGPU_HOST_CHUNKS, A/B only)
    int dense = DENSE_AUTO;            // the first launch's build (dense_mode, ALACGPU_DENSE)
    int pair_dense = -1;               // the paired kernel's form (ALACGPU_PAIR_DENSE): negative by batch size, 0 the 4-packet one, 1 the 8-packet one
    uint32_t* d_cu_arrivals = nullptr; // per-CU workgroup counters (alac_decode_params::cu_arrivals): ONE array per device, shared by
                                       // every context of the process on it (cu_counters_acquire), so that launches of different
                                       // contexts take their turns on a CU from the same counter
    // pairing: the switch (alacgpu_set_pairing), the context's own verdict (PAIR_WINDOW), the table, the device counters
    // (alac_decode_params::pair_stats) and their page-locked copy, and what the copy said when the window began
    bool pairing = true, pair_gave_up = false;
    alac_pair_entry* d_pair_table = nullptr;
    size_t pair_table_bytes = 0;
    unsigned long long* d_pair_stats = nullptr;
    unsigned long long* h_pair_stats = nullptr;
    unsigned long long* h_pair_stats_dev = nullptr;   // the copy's device-side address
    unsigned pair_launches = 0, pair_idle = 0;   // paired launches of the window; launches since the context gave up
    bool pair_first_window = true;
    unsigned long long pair_win[PAIR_COUNTERS] = {};
    bool zero_copy = true;             // host-buffer entry points store straight into page-locked output (ALACGPU_ZERO_COPY=0: A/B)
    // grow-only device workspace for the host-buffer entry points
    void* d_ws = nullptr;
    size_t ws_bytes = 0;
    int32_t* h_frame = nullptr;        // pinned staging of alacgpu_decode_frame (one slot of the widest kind)
    scratch enc;     // alacgpu_encode_device: per workgroup of a round alac_enc_items(smax) codes (buf[0]) and bit positions + 1 (buf[1])
    scratch scan;    // alacgpu_compact_packets_device, alacgpu_stage_packets_device: the partial sums of the scan's upper levels
    scratch norm;    // alacgpu_normalize_top_device: the maxima of the parts of every row, [rows, parts] floats
    scratch mix;     // alacgpu_mix_device: the sums of the squares of the signal and the noise over the parts of every row, [rows, parts, 2] floats
    scratch level;   // alacgpu_level_device: the sum of squares, the peak and the hop sums of every plane, [rows, channels, 2 + hops] doubles
    scratch reverb;  // alacgpu_reverb_device: the spectra of every block of the signal and partition of the impulse response of every row,
                     // [rows, units, ALAC_REVERB_N] float2, and behind them one alac_reverb_row per row (alac_reverb.h)
    void* d_reverb_twiddles = nullptr;   // alacgpu_reverb_device: exp(-2 pi i k / N), float2 [ALAC_REVERB_N], made at the first call
    void* h_reverb_twiddles = nullptr;   // ... and the page-locked table it is copied from on that call's stream
    scratch stretch; // alacgpu_time_stretch_device: the spectra of the STFT frames, [rows, channels, 1 + frames / hop, n_fft / 2 + 1] float2
                     // (buf[0]), and of the output frames, [rows, channels, alac_stretch_cap(out_frames), n_fft / 2 + 1] float2 (buf[1])
    scratch pyin;    // alacgpu_pyin_device: the log2 observations of every frame, [planes, frames, n_bins] voiced and [planes, frames] unvoiced and vp
                     // (buf[0]), and the decode's uint16 backpointers, [planes, frames, 2 n_bins] (buf[1])
    scratch kaldi_pitch;   // alacgpu_kaldi_pitch_device: the partial sums, the downsampled rows, the NCCF planes, the raw track and the
                     // epilogue's weights (buf[0], alac_kpitch_scratch of alac_kaldi_pitch.h), and the decode's uint16 backpointers,
                     // [planes, frames, n_states] (buf[1])
    void* d_stretch_tables[3] = {};      // alacgpu_time_stretch_device, for n_fft 512, 1024, 2048: exp(-2 pi i k / n_fft), float2 [n_fft], and
                                         // behind it the periodic Hann window, float [n_fft]; made at the first call with that n_fft
    void* h_stretch_tables[3] = {};      // ... and the page-locked tables they are copied from on that call's stream
    std::string last_error;
};

// A grow-only device buffer: when need_bytes exceed the have_bytes that p holds, p is freed and alloc_bytes allocated (the
// caller has waited for every user of the old buffer and chooses the slack).
template <class T>
int grow(alacgpu_ctx* ctx, T*& p, size_t& have_bytes, size_t need_bytes, size_t alloc_bytes) {
    if (need_bytes <= have_bytes) return ALACGPU_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    have_bytes = 0;
    HIP_TRY(ctx, hipMalloc((void**)&p, alloc_bytes));
    have_bytes = alloc_bytes;
    return ALACGPU_OK;
}

inline int scratch::acquire(alacgpu_ctx* ctx, hipStream_t stream, size_t need0, size_t alloc0, size_t need1, size_t alloc1) {
    held = need0 || need1;
    if (!held) return ALACGPU_OK;
    if (!done) HIP_TRY(ctx, hipEventCreateWithFlags(&done, hipEventDisableTiming));
    if (need0 > bytes[0] || need1 > bytes[1]) {
        if (used) HIP_TRY(ctx, hipEventSynchronize(done));       // the last call has finished with it
        const int rc = grow(ctx, buf[0], bytes[0], need0, alloc0);
        return rc ? rc : grow(ctx, buf[1], bytes[1], need1, alloc1);
    }
    if (used) HIP_TRY(ctx, hipStreamWaitEvent(stream, done, 0));   // (a call on another stream may still use it)
    return ALACGPU_OK;
}

inline int scratch::release(alacgpu_ctx* ctx, hipStream_t stream) {
    if (!held) return ALACGPU_OK;
    HIP_TRY(ctx, hipEventRecord(done, stream));
    used = true;
    held = false;
    return ALACGPU_OK;
}

// What a call that acquires a scratch declares in front of the acquire: a return between the acquire and the release (a launch
// that failed behind others that went out) still records the event on the call's stream, so the next call, whatever its
// stream, is ordered behind the launches that did go out.  Behind a release it does nothing; last_error stays the call's.
struct scratch_hold {
    scratch& s;
    hipStream_t stream;
    ~scratch_hold() {
        if (!s.held) return;
        if (s.done && hipEventRecord(s.done, stream) == hipSuccess) s.used = true;
        s.held = false;
    }
};

inline void scratch::destroy() {
    if (used) (void)hipEventSynchronize(done);
    if (done) (void)hipEventDestroy(done);
    for (void* b : buf) (void)hipFree(b);   // (a null pointer is a no-op)
}

// (alacgpu_api.hip)
uint32_t smax(const alacgpu_ctx* ctx);   // the longest frame any stream cfg declares, at most MAX_FRAME
bool pcm_view_ok(const void* d_pcm, uint32_t channels, int layout, int dtype, uint64_t plane_stride);
void* device_view_of_pinned(const void* host, size_t bytes);   // the device-side address of page-locked host memory, else null

#endif
