// alacgpu_ranges.h -- packet-range arithmetic shared by the host-buffer path (alacgpu_api.hip) and the multi-GPU part
// (alacgpu_comm.hip).  Plain C++ with no HIP in it, so that a host compiler can build it alone
// (tests/test_gather_plan.py drives it).
#pragma once
#include <cstdint>
#include <vector>

namespace alacgpu {

// Cut k of `parts` over n packets, rounded up to whole groups of 8 (the kernels work in groups of 8) and at most n:
// cut 0 is 0 and cut `parts` is n.
inline uint64_t group_cut(uint64_t n, uint64_t k, uint64_t parts) {
    const uint64_t c = (n * k / parts + 7u) & ~7ull;
    return c < n ? c : n;
}

enum gather_kind { GATHER_ALLGATHER, GATHER_SEND, GATHER_RECV, GATHER_BCAST };

// One collective call of a gather.  SEND / RECV: `peer` is the other rank and [first, first + count) the piece that
// travels.  BCAST: `peer` is the root, whose piece it is.  ALLGATHER: every rank's piece holds `count` packets, rank r's
// starting at first + r * count (peer is unused).
struct gather_op { gather_kind kind; int peer; uint64_t first, count; };

// the calls in issue order, and whether they go between GroupStart and GroupEnd
struct gather_plan_t { std::vector<gather_op> ops; bool grouped = false; };

// What rank `rank` of `world` issues to gather piece [first[r], first[r] + count[r]) of every rank r in place.  Equal pieces
// that lie side by side in rank order are one plain all-gather.  Any other pieces are exchanged in one group: in round k,
// each rank sends its piece to rank + k and receives the piece of rank - k, so every round pairs different ranks.  Without
// send / receive the group holds one broadcast per owner.  Empty pieces are skipped.
inline gather_plan_t gather_plan(int rank, int world, const uint64_t* first, const uint64_t* count, bool have_send_recv) {
    gather_plan_t plan;
    bool equal = true;
    for (int r = 0; r < world; r++) equal = equal && count[r] == count[0] && first[r] == first[0] + (uint64_t)r * count[0];
    if (equal) {   // (always so for one rank)
        if (count[0]) plan.ops.push_back({GATHER_ALLGATHER, -1, first[0], count[0]});
        return plan;
    }
    plan.grouped = true;
    if (have_send_recv) {
        for (int k = 1; k < world; k++) {
            const int to = (rank + k) % world, from = (rank - k + world) % world;
            if (count[rank]) plan.ops.push_back({GATHER_SEND, to, first[rank], count[rank]});
            if (count[from]) plan.ops.push_back({GATHER_RECV, from, first[from], count[from]});
        }
    } else {
        for (int r = 0; r < world; r++)
            if (count[r]) plan.ops.push_back({GATHER_BCAST, r, first[r], count[r]});
    }
    return plan;
}

}  // namespace alacgpu
