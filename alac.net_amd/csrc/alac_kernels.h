// alac_kernels.h -- launch parameters shared by the kernels and the C-ABI host code.
#ifndef ALAC_KERNELS_H
#define ALAC_KERNELS_H
#include <stdint.h>

// Same layout as alacgpu_cfg (include/alacgpu.h); kept separate so the kernels do not depend on the public header.
struct alacgpu_cfg_dev {
    uint32_t max_samples_per_frame;
    uint8_t sample_size, rice_history_mult, rice_initial_history, rice_kmodifier;
    uint8_t num_channels, ctor_sample_size, reserved, pad;
};
static_assert(sizeof(alacgpu_cfg_dev) == 12, "cfg layout");

// Same numbering as ALACGPU_ST_* (include/alacgpu.h)
enum {
    ALACGPU_ST_OK_D = 0,
    ALACGPU_ST_UNSUPPORTED_ELEMENT_D = 1,
    ALACGPU_ST_UNSUPPORTED_SAMPLE_SIZE_D = 2,
    ALACGPU_ST_UNSUPPORTED_PREDTYPE_D = 3,
    ALACGPU_ST_BAD_SAMPLE_COUNT_D = 4,
    ALACGPU_ST_OVERRUN_D = 5,
    ALACGPU_ST_REF_THROWS_D = 6,
    ALACGPU_ST_UNSUPPORTED_PARAMS_D = 7,
    ALACGPU_ST_DEST_RANGE_D = 8
};

// One entry of the pairing table, 16 bytes, written and read as one vector: the tag -- the packet's device address (48 bits), its
// size (its low 16 bits beside the address, all of it in the hash) and a hash of the size and the packet's first 16 bytes --
// and the bit position, from the 16-byte aligned-down packet start, at which channel B's Rice stream starts.  An entry that is
// torn, stale or from another packet costs a decode (the paired kernel verifies the start), never a wrong result.
struct alac_pair_entry { uint32_t addr_lo, addr_hi_size, hash, start; };
static_assert(sizeof(alac_pair_entry) == 16, "one vector store per entry");
enum { PAIR_COUNTERS = 5 };       // alac_decode_params::pair_stats
enum { PAIR_WAYS = 8 };           // entries per set of the pairing table: one 128-byte line, looked at by 8 lanes at once
enum { AB_FLAG_PAIR_LEFT = 8 };   // alac_decode_params::ab_flags: the paired kernel left packets of this group undecoded

struct alac_decode_params {
    const uint8_t* blob;        // 16-byte aligned
    uint64_t blob_limit;        // readable bytes from blob (blob_bytes rounded up to 16)
    const uint64_t* offsets;
    const uint32_t* sizes;
    const uint16_t* cfg_idx;    // may be null
    const alacgpu_cfg_dev* cfgs;
    uint32_t n_cfgs;
    uint32_t n_packets;
    int32_t* pcm_out;
    uint32_t slot_ints;
    int32_t* out_bytes;         // may be null
    int32_t* out_samples;       // may be null
    int32_t* status;
    uint32_t out_format;        // 0: one int32 per sample; 1: packed little-endian PCM bytes (FormatSamples fused)
    // Where channel A of a two-channel packet waits between the two passes: null = in the packet's own output slot (ints
    // [n, 2n)); else packet p's place is park + p * park_stride (>= n ints each).  The host-buffer entry point uses a place
    // of its own when pcm_out is page-locked HOST memory the kernels store into directly: the parked samples are read back,
    // and a read across the link costs what the whole decode costs.
    int32_t* park;
    uint32_t park_stride;
#ifdef ALAC_DIAG
    unsigned long long* dbg;    // diagnostic build (make diag) only: 8 stamps per workgroup, see alac_diag.h
#endif
    // alac_decode_ab_kernel, then alac_decode_ab32_kernel: flag g covers packets 8g .. 8g+7.  The first writes 0 where it
    // decoded the group and 1 where it did not; the second decodes the groups flagged 1 and writes 2 there.  One array per
    // launch pair in flight (the host keeps a pool, alacgpu_api.hip: launch_slot).
    // With a paired kernel in front (pair_ran): it sets the flag of a group of which it left packets (four or all eight) undecoded to
    // AB_FLAG_PAIR_LEFT (the flags are zeroed in front of it); alac_decode_ab_small_kernel then decodes the groups flagged so,
    // all eight packets, and leaves the others alone (their flag stays 0).
    uint32_t* ab_flags;
    // Two-pass kernels: one counter per CU (index: XCC_ID, SE_ID, SH_ID, CU_ID), bumped by every workgroup that starts
    // there; its value, the workgroup's turn on the CU, rotates the roles of the workgroup's waves over the SIMDs.
    // 2048 entries, never reset (only the value modulo 4 matters).  Null: roles in wave order.
    uint32_t* cu_arrivals;
    // Destination mode (alacgpu_decode_into_device); dst_first == null: the slot layout above, and the rest is unused.
    // Packet p's frame i, channel c goes to element (dst_first[p] + i) * channels + c (layout 0, interleaved) or
    // c * plane_stride + dst_first[p] + i (layout 1, planar) of pcm_out, as int32 (dtype 0) or as float32 sample * 2^-(ss-1)
    // (dtype 1); frames i >= dst_frames[p] are not stored.  A run outside [0, out_elems) or a stream cfg with another channel
    // count is status ALACGPU_ST_DEST_RANGE_D, and such a packet writes nothing.  slot_ints is channels * Smax (the statuses
    // of the slot layout) and channel A is parked at park + p * park_stride.
    // src_skip (may be null: no skip): a window of the packet -- frames i with src_skip[p] <= i < src_skip[p] + dst_frames[p]
    // are stored, frame i at dst_first[p] + (i - src_skip[p]).  With src_skip, dst_first is the launch's own copy from
    // alac_window_first_kernel: a skip above 16384 there turns into a run that does not fit (status ALACGPU_ST_DEST_RANGE_D).
    const uint64_t* dst_first;
    const uint32_t* dst_frames;
    const uint32_t* src_skip;
    uint64_t out_elems;
    uint64_t plane_stride;
    uint32_t channels, layout, dtype;
    // Pairing (alac_decode_ab_pair_kernel): where channel B of a two-channel packet starts, remembered from
    // an earlier decode of the same packet.  pair_table: pair_mask + 1 sets (a power of two) of PAIR_WAYS entries, null
    // in calls that neither read nor write it; the two-pass kernels write an entry per compressed two-channel packet, the paired
    // kernel reads them.  pair_stats: PAIR_COUNTERS device counters -- packets the paired kernel finished with a verified start,
    // packets it found no entry for, packets whose remembered start was wrong, workgroups that left their packets to the launch
    // behind (for any reason), groups of 4 packets that workgroups finished (one per workgroup of the 4-packet kernel, two per
    // workgroup of the 8-packet one: a packet that sends its workgroup away weighs the same in both); pair_stats_host: their page-locked copy, brought up
    // to date by the launch behind the paired kernel.  pair_ran: the paired kernel ran in front of this launch.
    alac_pair_entry* pair_table;
    uint32_t pair_mask;
    uint32_t pair_ran;
    unsigned long long* pair_stats;
    unsigned long long* pair_stats_host;
};

#ifdef __HIPCC__
// two passes (channel A, then B), 8 packets / 256-thread workgroup (three working waves), LPC orders 1..8
extern "C" __global__ void alac_decode_ab_kernel(alac_decode_params p);
extern "C" __global__ void alac_decode_ab5_kernel(alac_decode_params p);         // the same with 96 registers (five workgroups per CU)
extern "C" __global__ void alac_decode_ab_small_kernel(alac_decode_params p);   // the same with 16-step units (batches up to 4096 packets)
// one pass, 4 packets / workgroup, both channels of a packet side by side from a remembered start of channel B; in front of
// alac_decode_ab_small_kernel, which decodes what this one leaves
extern "C" __global__ void alac_decode_ab_pair_kernel(alac_decode_params p);
// the same on the dense layout: 8 packets x 2 channels / workgroup (one entropy wave with 4 lanes per stream, two FIR waves)
extern "C" __global__ void alac_decode_ab_pair_dense_kernel(alac_decode_params p);
// test hook (alacgpu_pairing_shift_starts): every remembered start + 1
extern "C" __global__ void alac_pair_shift_kernel(alac_pair_entry* table, uint32_t entries);
// the second launch, for the groups of 8 packets the first one flagged: two taps per lane of the FIR wave (orders 9..16) or
// four (any order, delta mode, order 0)
extern "C" __global__ void alac_decode_ab32_kernel(alac_decode_params p);
// the first launch with 16 packets / 256-thread workgroup (one entropy wave for 16 streams, orders 1..16): big batches
extern "C" __global__ void alac_decode_ab_dense_kernel(alac_decode_params p);
// the window builds of the five above, for the calls with src_skip (only their output wave differs)
extern "C" __global__ void alac_decode_ab_win_kernel(alac_decode_params p);
extern "C" __global__ void alac_decode_ab5_win_kernel(alac_decode_params p);
extern "C" __global__ void alac_decode_ab_small_win_kernel(alac_decode_params p);
extern "C" __global__ void alac_decode_ab32_win_kernel(alac_decode_params p);
extern "C" __global__ void alac_decode_ab_dense_win_kernel(alac_decode_params p);
// destination mode only, behind the launch pair: the zeros of every run (frames past a packet's decoded ones, the whole run of
// a packet that failed)
extern "C" __global__ void alac_dst_fill_kernel(alac_decode_params p);
// window calls only, in front of the launch pair: first[p] = dst_first[p], or ~0 (a run that never fits) where src_skip[p] > 16384
extern "C" __global__ void alac_window_first_kernel(const uint64_t* dst_first, const uint32_t* src_skip, uint64_t* first,
                                                    uint32_t n_packets);
#endif

#endif
