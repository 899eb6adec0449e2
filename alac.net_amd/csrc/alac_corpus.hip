// alac_corpus.hip -- the crop planner: window_plan (alac.net_amd/__init__.py) for B crops at once against a corpus's packet
// tables in HBM.  It writes the per-packet arrays alacgpu_decode_window_into_device reads, so a step of random crops needs
// nothing from the host but (file, first frame) pairs.
//
// One wave per crop.  The crop's facts (file, packet range, the two searches) are wave-uniform; the searches are 64-ary:
// every step the 64 lanes probe the ends of 64 equal parts of the range with one load and a ballot picks the part, so a file
// of up to 4096 packets takes two dependent loads per search and one of 262144 three (a binary search: 12 and 18).  Then the
// lanes stride over the crop's K entries: neighbouring lanes read neighbouring packets of the tables and write neighbouring
// entries of the six arrays.  Every output element has exactly one writer; all stores are plain vector stores.
#include "alac_corpus.h"

namespace {

// The first index i in [lo, hi) with a[i] > v (UPPER) or a[i] >= v (!UPPER), hi if there is none; a ascending over the range.
// lo, hi and v are wave-uniform, and so is the result.  Every lane of the wave must be active.
template <bool UPPER>
__device__ __forceinline__ uint32_t wave_search(const uint64_t* __restrict__ a, uint32_t lo, uint32_t hi, uint64_t v, uint32_t lane) {
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63u) >> 6;
        // lane l probes the last element of part l (parts of `step` elements); a probe past the range counts as a hit
        const uint64_t j = (uint64_t)lo + (uint64_t)(lane + 1u) * step - 1u;
        bool hit = true;
        if (j < hi) {
            const uint64_t e = a[j];
            hit = UPPER ? e > v : e >= v;
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(hit);
        if (mask == 0) return hi;                       // (only when the 64 parts cover the range exactly)
        const uint32_t k = (uint32_t)__builtin_ctzll(mask);
        const uint64_t top = (uint64_t)lo + (uint64_t)(k + 1u) * step - 1u;   // the probe that hit: the answer is at most there
        lo += k * step;                                  // the probe in front of it missed: the answer is past it
        if (step == 1u) return lo;
        hi = top < hi ? (uint32_t)top : hi;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(ALAC_PLAN_THREADS) void alac_plan_crops_kernel(alac_plan_params p) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t b64 = (uint64_t)blockIdx.x * (ALAC_PLAN_THREADS / 64) + wave;
    if (b64 >= p.n_crops) return;                        // (wave-uniform: whole waves leave)
    const uint32_t b = (uint32_t)b64;
    const uint32_t K = p.entries_per_crop;
    const uint32_t f = p.crop_file[b];
    const uint64_t o = p.crop_offset[b];

    // the crop's file and length: -1 for a file or an offset that does not exist
    int64_t length = -1;
    uint32_t g0 = 0, n = 0;
    uint32_t cfg = ALAC_PLAN_PAD_CFG;
    if (f < p.n_files) {
        g0 = p.file_first[f];
        n = p.file_first[f + 1u] - g0;
        const uint64_t total = n ? p.pkt_end[g0 + n - 1u] : 0u;
        if (o <= total) {
            const uint64_t left = total - o;
            length = (int64_t)(left < p.crop_frames ? left : (uint64_t)p.crop_frames);
            cfg = p.file_cfg[f];
        }
    }
    // window_plan: packets p0 .. p1 of the file.  p0: the first packet that ends past o (packet 0 for a window from frame 0);
    // p1: one past the last packet that starts in front of the window's end -- packet i > 0 starts at pkt_end[i - 1].
    const uint64_t end = o + (uint64_t)(length > 0 ? length : 0);
    uint32_t p0 = 0, p1 = 0;
    if (length > 0 && n > 0) {
        const uint64_t* const ends = p.pkt_end + g0;
        p0 = o == 0 ? 0u : wave_search<true>(ends, 0u, n, o, lane);
        const uint32_t q = wave_search<false>(ends, 0u, n - 1u, end, lane) + 1u;
        p1 = q > p0 ? q : p0;
    }
    uint32_t count = p1 - p0;
    if (count > K) {                                     // the caller's K is too small: a length code, and padding only
        length = -2;
        count = 0;
    }
    if (lane == 0) p.lengths[b] = length;

    const uint64_t row = (uint64_t)b * p.dst_stride;
    const uint64_t j0 = (uint64_t)b * K;                 // (n_crops * K fits 32 bits: the host checks)
    for (uint32_t i = lane; i < K; i += 64u) {
        uint64_t off = 0, first = 0;
        uint32_t size = 0, frames = 0, skip = 0;
        uint16_t ci = (uint16_t)ALAC_PLAN_PAD_CFG;
        if (i < count) {
            const uint32_t local = p0 + i;               // the packet's index in its file (< n)
            const uint64_t g = (uint64_t)g0 + local;
            const uint64_t start = local ? p.pkt_end[g - 1u] : 0u;
            const uint64_t stop = p.pkt_end[g];
            const uint64_t lo = start > o ? start : o;
            const uint64_t hi = stop < end ? stop : end;
            frames = hi > lo ? (uint32_t)(hi - lo) : 0u;
            first = row + (lo - o);
            const uint64_t s = lo - start;
            skip = s < ALAC_PLAN_MAX_SKIP ? (uint32_t)s : ALAC_PLAN_MAX_SKIP;
            off = p.pkt_offset[g];
            size = p.pkt_size[g];
            ci = (uint16_t)cfg;
        }
        p.offsets[j0 + i] = off;
        p.sizes[j0 + i] = size;
        p.cfg_idx[j0 + i] = ci;
        p.dst_first[j0 + i] = first;
        p.dst_frames[j0 + i] = frames;
        p.src_skip[j0 + i] = skip;
    }
}
