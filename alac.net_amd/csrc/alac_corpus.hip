// alac_corpus.hip -- the crop planner: window_plan (alac.net_amd/__init__.py) for B crops at once against a corpus's packet
// tables in HBM.  It writes the per-packet arrays alacgpu_decode_window_into_device reads, so a step of random crops needs
// nothing from the host but (file, first frame) pairs.  alac_plan_crops_frames_kernel is the same wave with a window length
// per crop (the crops of files of different sample rates need different numbers of source frames).
//
// One wave per crop.  The crop's facts (file, packet range, the two searches) are wave-uniform; the searches are 64-ary:
// every step the 64 lanes probe the ends of 64 equal parts of the range with one load and a ballot picks the part, so a file
// of up to 4096 packets takes two dependent loads per search and one of 262144 three (a binary search: 12 and 18).  Then the
// lanes stride over the crop's K entries: neighbouring lanes read neighbouring packets of the tables and write neighbouring
// entries of the six arrays.  Every output element has exactly one writer; all stores are plain vector stores.
//
// Behind it, the packet compaction (alacgpu_compact_packets_device): what brings the encoder's packets -- packet p in its own
// slot at p * slot_bytes -- into the resident layout, back to back.  An exclusive scan of the sizes gives pkt_offset; it is
// hierarchical in separate launches (sums of tiles of 2048, the scan of those sums, the scan of the tiles on top of it: three
// levels reach 2^33 packets), so no workgroup ever waits for another.  The copy is spread over the DESTINATION bytes, not
// over the packets: a thread owns 16-byte aligned chunks of the blob, finds the packet a chunk lies in with a binary search
// of pkt_offset (narrowed to the tile's packets first) and, when the whole chunk belongs to one packet, stores it with one
// 16-byte store built from two aligned 16-byte loads of the slot (v_alignbyte); a chunk with a packet boundary in it goes
// dword by dword the same way, and only the dwords that hold a boundary themselves byte by byte.  So 11 KB packets move at 16
// bytes per lane and a batch of 10-byte packets still fills its waves.  Nothing outside the copied packets is stored to.
//
// And the packet staging (alacgpu_stage_packets_device): the gather of a plan's packets out of a corpus that lies partly in
// page-locked host memory into a small blob in HBM, each packet at the next multiple of 16.  The same scan (a size counts
// rounded up to 16, or as 0 when the packet does not lie inside one of the two parts) and the same copy over destination
// chunks, but shaped for the link: a thread first finds the sources of all its chunks of a tile, then issues every load of
// them -- up to 2 * ALAC_STAGE_CHUNKS independent 16-byte loads per lane -- and only then combines and stores.  Every
// destination chunk is one packet's, so there is no dword or byte path.
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

// EACH: every crop has a window length of its own, p.crop_frames_each[b], and p.crop_frames is their bound
// (alacgpu_plan_crops_frames_device)
template <bool EACH>
__device__ __forceinline__ void plan_crops(const alac_plan_params& p) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t b64 = (uint64_t)blockIdx.x * (ALAC_PLAN_THREADS / 64) + wave;
    if (b64 >= p.n_crops) return;                        // (wave-uniform: whole waves leave)
    const uint32_t b = (uint32_t)b64;
    const uint32_t K = p.entries_per_crop;
    const uint32_t f = p.crop_file[b];
    const uint64_t o = p.crop_offset[b];
    uint32_t frames_b = p.crop_frames;
    bool fits = true;
    if constexpr (EACH) {                                // a window longer than the bound would leave its row: no such crop
        frames_b = p.crop_frames_each[b];
        fits = frames_b <= p.crop_frames;
    }

    // the crop's file and length: -1 for a file or an offset that does not exist
    int64_t length = -1;
    uint32_t g0 = 0, n = 0;
    uint32_t cfg = ALAC_PLAN_PAD_CFG;
    if (f < p.n_files && fits) {
        g0 = p.file_first[f];
        n = p.file_first[f + 1u] - g0;
        const uint64_t total = n ? p.pkt_end[g0 + n - 1u] : 0u;
        if (o <= total) {
            const uint64_t left = total - o;
            length = (int64_t)(left < frames_b ? left : (uint64_t)frames_b);
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

}  // namespace

__global__ __launch_bounds__(ALAC_PLAN_THREADS) void alac_plan_crops_kernel(alac_plan_params p) { plan_crops<false>(p); }
__global__ __launch_bounds__(ALAC_PLAN_THREADS) void alac_plan_crops_frames_kernel(alac_plan_params p) { plan_crops<true>(p); }

// ---- packet compaction -----------------------------------------------------------------------------------------------------------
namespace {

// a size above the slot counts as 0: whatever the device data say, no read leaves a slot
__device__ __forceinline__ uint64_t counted(uint32_t size, uint64_t slot_bytes) { return size <= slot_bytes ? size : 0u; }
__device__ __forceinline__ uint64_t counted(uint64_t sum, uint64_t) { return sum; }

// staging: a packet counts, rounded up to 16, when it lies wholly inside one of the two parts of the source space (offsets
// below lo_bytes: the first part).  Whatever the device data say, no read leaves the parts
__device__ __forceinline__ uint64_t staged(uint32_t size, uint64_t off, uint64_t lo_bytes, uint64_t hi_bytes) {
    const bool in_lo = off < lo_bytes && size <= lo_bytes - off;
    const bool in_hi = off >= lo_bytes && off - lo_bytes <= hi_bytes && size <= hi_bytes - (off - lo_bytes);
    return in_lo || in_hi ? ((uint64_t)size + 15u) & ~(uint64_t)15 : 0u;
}

// The thread's ALAC_SCAN_ITEMS consecutive elements of the tile (0 behind n) and their sum.
template <bool STAGE, class T>
__device__ __forceinline__ uint64_t scan_load(const alac_scan_params<T>& p, uint64_t first, uint64_t (&v)[ALAC_SCAN_ITEMS]) {
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < ALAC_SCAN_ITEMS; i++) {
        v[i] = 0u;
        if (first + i < p.n) {
            if constexpr (STAGE) v[i] = staged(p.in[first + i], p.src_offset[first + i], p.lo_bytes, p.hi_bytes);
            else v[i] = counted(p.in[first + i], p.slot_bytes);
        }
        sum += v[i];
    }
    return sum;
}

// The sum of `v` over the threads in front of this one, and over the whole workgroup in `total`.
__device__ __forceinline__ uint64_t block_exclusive(uint64_t v, uint64_t& total) {
    __shared__ uint64_t wave_sum[ALAC_SCAN_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63u) wave_sum[wave] = inc;
    __syncthreads();
    uint64_t front = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < ALAC_SCAN_THREADS / 64; w++) {
        if (w < wave) front += wave_sum[w];
        total += wave_sum[w];
    }
    return front + inc - v;
}

template <bool STAGE, class T>
__device__ __forceinline__ void scan_sums(const alac_scan_params<T>& p) {
    uint64_t v[ALAC_SCAN_ITEMS], total;
    const uint64_t sum = scan_load<STAGE>(p, (uint64_t)blockIdx.x * ALAC_SCAN_TILE + (uint64_t)threadIdx.x * ALAC_SCAN_ITEMS, v);
    (void)block_exclusive(sum, total);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = total;
}

template <bool STAGE, class T>
__device__ __forceinline__ void scan_tiles(const alac_scan_params<T>& p) {
    uint64_t v[ALAC_SCAN_ITEMS], total;
    const uint64_t first = (uint64_t)blockIdx.x * ALAC_SCAN_TILE + (uint64_t)threadIdx.x * ALAC_SCAN_ITEMS;
    const uint64_t sum = scan_load<STAGE>(p, first, v);          // (every load of the tile is in front of the barrier: in == out is safe)
    const uint64_t front = p.tile_base ? p.tile_base[blockIdx.x] : 0u;
    uint64_t run = p.add + front + block_exclusive(sum, total);
#pragma unroll
    for (uint32_t i = 0; i < ALAC_SCAN_ITEMS; i++) {
        if (first + i < p.n) p.out[first + i] = run;
        run += v[i];
    }
    if (p.total && blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) p.total[0] = front + total;
}

// The last packet of lo .. hi (both inclusive) whose offset is at most x; pkt_offset[lo] <= x.  Behind packets of size 0,
// which share their offset with the next one, this is the packet that owns byte x (for x in front of the end of all packets).
__device__ __forceinline__ uint32_t find_packet(const uint64_t* __restrict__ pkt_offset, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (pkt_offset[mid] <= x) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// Sixteen bytes from byte r (0 .. 15) of the 32 bytes v0, v1
__device__ __forceinline__ uint4 align16(uint4 v0, uint4 v1, uint32_t r) {
    const bool k2 = (r & 8u) != 0, k1 = (r & 4u) != 0;
    const uint32_t a0 = k2 ? v0.z : v0.x, a1 = k2 ? v0.w : v0.y, a2 = k2 ? v1.x : v0.z, a3 = k2 ? v1.y : v0.w;
    const uint32_t a4 = k2 ? v1.z : v1.x, a5 = k2 ? v1.w : v1.y;
    const uint32_t b0 = k1 ? a1 : a0, b1 = k1 ? a2 : a1, b2 = k1 ? a3 : a2, b3 = k1 ? a4 : a3, b4 = k1 ? a5 : a4;
    const uint32_t j = r & 3u;
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(b1, b0, j);
    o.y = __builtin_amdgcn_alignbyte(b2, b1, j);
    o.z = __builtin_amdgcn_alignbyte(b3, b2, j);
    o.w = __builtin_amdgcn_alignbyte(b4, b3, j);
    return o;
}

struct packet_span {
    uint64_t begin, end;          // the packet's bytes as positions (blob offset + shift)
    const uint8_t* src;           // its slot
    bool fits;                    // ... and whether it is copied at all
};

__device__ __forceinline__ packet_span span_of(const alac_copy_params& p, uint32_t lo, uint32_t hi, uint64_t q, uint32_t shift) {
    const uint32_t k = find_packet(p.pkt_offset, lo, hi, q - shift);
    const uint64_t off = p.pkt_offset[k], size = counted(p.sizes[k], p.slot_bytes);
    packet_span s;
    s.begin = off + shift;
    s.end = s.begin + size;
    s.src = p.packets + (uint64_t)k * p.slot_bytes;
    s.fits = off + size <= p.capacity;
    return s;
}

// The 16-byte chunk of the blob at position q0 (a multiple of 16); positions lie `shift` in front of blob offsets so that they
// are aligned as the addresses are.  q_lo .. q_hi: the positions of all packet bytes in front of the capacity.
__device__ __forceinline__ void copy_chunk(const alac_copy_params& p, uint64_t q0, uint64_t q_lo, uint64_t q_hi, uint32_t shift,
                                           uint32_t lo, uint32_t hi) {
    const uint64_t a = q0 > q_lo ? q0 : q_lo, b = q0 + 16u < q_hi ? q0 + 16u : q_hi;
    if (a >= b) return;
    packet_span s = span_of(p, lo, hi, a, shift);
    if (q0 >= s.begin && q0 + 16u <= s.end) {            // the whole chunk is one packet's: one store
        if (!s.fits) return;
        const uint64_t at = q0 - s.begin;                // (at + 16 <= size <= slot_bytes)
        const uint32_t r = (uint32_t)at & 15u;
        const uint4* v = (const uint4*)(s.src + (at - r));
        const uint4 v0 = v[0];
        uint4 v1 = make_uint4(0u, 0u, 0u, 0u);
        if (r) v1 = v[1];                                // at - r + 16 < at + 16 <= slot_bytes, a multiple of 16: inside the slot
        *(uint4*)(p.blob + (q0 - shift)) = align16(v0, v1, r);
        return;
    }
    for (uint32_t d = 0; d < 4u; d++) {                  // a packet starts or ends in the chunk: dword by dword
        const uint64_t dq = q0 + 4u * d;
        const uint64_t da = dq > a ? dq : a, db = dq + 4u < b ? dq + 4u : b;
        if (da >= db) continue;
        if (da >= s.end) s = span_of(p, lo, hi, da, shift);
        if (dq >= s.begin && dq + 4u <= s.end) {
            if (!s.fits) continue;
            const uint64_t at = dq - s.begin;
            const uint32_t j = (uint32_t)at & 3u;
            const uint32_t* w = (const uint32_t*)(s.src + (at - j));
            const uint32_t w0 = w[0];
            const uint32_t w1 = j ? w[1] : 0u;           // at - j + 4 < at + 4 <= slot_bytes: inside the slot
            *(uint32_t*)(p.blob + (dq - shift)) = __builtin_amdgcn_alignbyte(w1, w0, j);
            continue;
        }
        for (uint64_t q = da; q < db; q++) {             // the dword holds a boundary: its bytes one by one
            if (q >= s.end) s = span_of(p, lo, hi, q, shift);
            if (s.fits) p.blob[q - shift] = s.src[q - s.begin];
        }
    }
}

// Where the 16-byte chunk at position q of the staging blob comes from: v, the aligned 16 bytes of the source that hold its
// first byte (null: the chunk is not copied), r, that byte's place in them, and whether the 16 bytes behind v hold bytes of
// the packet too.  lo .. hi: the tile's packets.
struct stage_src {
    const uint4* v;
    uint32_t r;
    bool two;
};

__device__ __forceinline__ stage_src stage_locate(const alac_stage_params& p, uint64_t q, uint64_t q_hi, uint32_t lo, uint32_t hi) {
    stage_src s;
    s.v = nullptr;
    s.r = 0;
    s.two = false;
    if (q >= q_hi) return s;
    const uint32_t k = find_packet(p.stage_offset, lo, hi, q);
    const uint64_t off = p.stage_offset[k], src = p.src_offset[k];
    const uint32_t size = p.sizes[k];
    const uint64_t room = staged(size, src, p.lo_bytes, p.hi_bytes);     // 0, or the packet lies inside one part
    const uint64_t at = q - off;                                         // (off <= q < capacity)
    if (at >= room || room > p.capacity - off) return s;                 // a packet that does not fit is not copied at all
    const bool in_lo = src < p.lo_bytes;
    const uint64_t from = (in_lo ? src : src - p.lo_bytes) + at;         // at < size: a byte of the packet
    s.r = (uint32_t)from & 15u;
    s.v = (const uint4*)((in_lo ? p.lo : p.hi) + (from - s.r));
    s.two = s.r != 0 && 16u - s.r < size - at;                           // only then v[1] holds a byte of the packet: inside the part
    return s;
}

}  // namespace

__global__ __launch_bounds__(ALAC_SCAN_THREADS) void alac_scan_sums_u32_kernel(alac_scan_params<uint32_t> p) { scan_sums<false>(p); }
__global__ __launch_bounds__(ALAC_SCAN_THREADS) void alac_scan_sums_u64_kernel(alac_scan_params<uint64_t> p) { scan_sums<false>(p); }
__global__ __launch_bounds__(ALAC_SCAN_THREADS) void alac_scan_tiles_u32_kernel(alac_scan_params<uint32_t> p) { scan_tiles<false>(p); }
__global__ __launch_bounds__(ALAC_SCAN_THREADS) void alac_scan_tiles_u64_kernel(alac_scan_params<uint64_t> p) { scan_tiles<false>(p); }
__global__ __launch_bounds__(ALAC_SCAN_THREADS) void alac_scan_sums_stage_kernel(alac_scan_params<uint32_t> p) { scan_sums<true>(p); }
__global__ __launch_bounds__(ALAC_SCAN_THREADS) void alac_scan_tiles_stage_kernel(alac_scan_params<uint32_t> p) { scan_tiles<true>(p); }

__global__ __launch_bounds__(ALAC_COPY_THREADS) void alac_compact_copy_kernel(alac_copy_params p) {
    __shared__ uint32_t range[2];
    const uint32_t shift = (uint32_t)((uintptr_t)p.blob & 15u);
    const uint64_t end = p.base + p.total[0];
    const uint64_t q_lo = p.base + shift, q_hi = (end < p.capacity ? end : p.capacity) + shift;
    const uint64_t q_first = q_lo & ~(uint64_t)15;
    for (uint64_t t = blockIdx.x;; t += gridDim.x) {     // tiles of the destination; every condition here is workgroup-uniform
        const uint64_t tq = q_first + t * ALAC_COPY_TILE;
        if (tq >= q_hi) break;
        if (threadIdx.x == 0) {                          // the tile's packets: the searches below stay among them
            const uint64_t a = tq > q_lo ? tq : q_lo, b = tq + ALAC_COPY_TILE < q_hi ? tq + ALAC_COPY_TILE : q_hi;
            range[0] = find_packet(p.pkt_offset, 0u, p.n_packets - 1u, a - shift);
            range[1] = find_packet(p.pkt_offset, range[0], p.n_packets - 1u, b - 1u - shift);
        }
        __syncthreads();
        const uint32_t lo = range[0], hi = range[1];
#pragma unroll
        for (uint32_t c = 0; c < ALAC_COPY_CHUNKS; c++)
            copy_chunk(p, tq + ((uint64_t)c * ALAC_COPY_THREADS + threadIdx.x) * 16u, q_lo, q_hi, shift, lo, hi);
        __syncthreads();
    }
}

__global__ __launch_bounds__(ALAC_STAGE_THREADS) void alac_stage_copy_kernel(alac_stage_params p) {
    __shared__ uint32_t range[2];
    const uint64_t total = p.total[0];
    const uint64_t q_hi = total < p.capacity ? total : p.capacity;
    const uint64_t tiles = q_hi / ALAC_STAGE_TILE + (q_hi % ALAC_STAGE_TILE ? 1u : 0u);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {      // tiles of the destination; the bound is workgroup-uniform
        const uint64_t tq = t * ALAC_STAGE_TILE;
        if (threadIdx.x < 64u) {                         // the first wave, whole: the tile's packets, by two 64-ary searches
            const uint64_t last = (q_hi - tq < ALAC_STAGE_TILE ? q_hi : tq + ALAC_STAGE_TILE) - 1u;
            const uint32_t lo = wave_search<true>(p.stage_offset, 0u, p.n_packets, tq, threadIdx.x) - 1u;     // (stage_offset[0] is 0)
            const uint32_t hi = wave_search<true>(p.stage_offset, lo, p.n_packets, last, threadIdx.x) - 1u;
            if (threadIdx.x == 0) {
                range[0] = lo;
                range[1] = hi;
            }
        }
        __syncthreads();
        const uint32_t lo = range[0], hi = range[1];
        // every source first, then every load, then the stores: the loads of all chunks are in flight together
        stage_src s[ALAC_STAGE_CHUNKS];
        uint4 v0[ALAC_STAGE_CHUNKS], v1[ALAC_STAGE_CHUNKS];
#pragma unroll
        for (uint32_t c = 0; c < ALAC_STAGE_CHUNKS; c++)
            s[c] = stage_locate(p, tq + ((uint64_t)c * ALAC_STAGE_THREADS + threadIdx.x) * 16u, q_hi, lo, hi);
#pragma unroll
        for (uint32_t c = 0; c < ALAC_STAGE_CHUNKS; c++) {
            v0[c] = v1[c] = make_uint4(0u, 0u, 0u, 0u);
            if (s[c].v) v0[c] = s[c].v[0];
            if (s[c].two) v1[c] = s[c].v[1];
        }
#pragma unroll
        for (uint32_t c = 0; c < ALAC_STAGE_CHUNKS; c++)
            if (s[c].v) *(uint4*)(p.stage + tq + ((uint64_t)c * ALAC_STAGE_THREADS + threadIdx.x) * 16u) = align16(v0[c], v1[c], s[c].r);
        __syncthreads();
    }
}
