"""The send / receive plan of the multi-GPU gather (alacgpu_ranges.h: gather_plan, group_cut), checked on the CPU over every
rank of worlds of 1 to 8: a small driver built against the header with the host compiler prints what each rank would issue,
and the plans of all ranks together must deliver every piece once, with every send met by its receive."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alac.net_amd", "csrc")
ALLGATHER, SEND, RECV, BCAST = 0, 1, 2, 3

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "alacgpu_ranges.h"
// stdin: "C n k parts" -> group_cut;  "P rank world have_send_recv first_0 count_0 ... " -> grouped, then kind peer first count
int main() {
    char tag;
    while (std::scanf(" %c", &tag) == 1) {
        if (tag == 'C') {
            unsigned long long n, k, parts;
            if (std::scanf("%llu %llu %llu", &n, &k, &parts) != 3) return 1;
            std::printf("%llu\n", (unsigned long long)alacgpu::group_cut(n, k, parts));
            continue;
        }
        int rank, world, sr;
        if (tag != 'P' || std::scanf("%d %d %d", &rank, &world, &sr) != 3) return 1;
        std::vector<uint64_t> first(world), count(world);
        for (int r = 0; r < world; r++) {
            unsigned long long f, c;
            if (std::scanf("%llu %llu", &f, &c) != 2) return 1;
            first[r] = f;
            count[r] = c;
        }
        const alacgpu::gather_plan_t plan = alacgpu::gather_plan(rank, world, first.data(), count.data(), sr != 0);
        std::printf("%d", plan.grouped ? 1 : 0);
        for (const alacgpu::gather_op& op : plan.ops)
            std::printf(" %d %d %llu %llu", (int)op.kind, op.peer, (unsigned long long)op.first, (unsigned long long)op.count);
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return r.stdout.splitlines()

    return run


def _sizes():
    """Packet byte sizes: uniform, and skewed like cfg5 (1-sample packets, uncompressed ones and 24-bit order-30 ones)."""
    rng = np.random.default_rng(5)
    out = [np.full(n, 4000, np.uint32) for n in (0, 1, 5, 8, 13, 64, 100, 1000)]
    for n in (9, 40, 333, 2048):
        kind = rng.integers(0, 3, n)
        out.append(np.where(kind == 0, 8, np.where(kind == 1, 16400, rng.integers(3000, 9000, n))).astype(np.uint32))
    skew = np.full(512, 10, np.uint32)
    skew[:16] = 200000                       # nearly all bytes up front: the byte-balanced cut leaves ranks empty
    out.append(skew)
    return out


def _cases(driver):
    """(first[W], count[W]) of every gather alacgpu_allgather_pcm / alacgpu_decode_allgather_device would make: shards by
    count and by bytes (the library's alacgpu_shard_ranges and its Python twin), cut into 1..4 pieces as
    alacgpu_decode_allgather_device cuts them."""
    import alac.net_amd as pkg
    from alac.net_amd import sharding

    shards = set()
    for world in range(1, 9):
        for sizes in _sizes():
            for first in (pkg.shard_ranges(sizes, world), sharding.shard_ranges(sizes, world)):
                shards.add(tuple(int(x) for x in first))
            n = len(sizes)
            shards.add(tuple(min(n, (n * r // world + 7) & ~7) for r in range(world)) + (n,))
    queries = sorted({(s[r + 1] - s[r], k, parts) for s in shards for r in range(len(s) - 1) for parts in range(1, 5)
                      for k in range(parts + 1)})
    cut = dict(zip(queries, (int(x) for x in driver([f"C {n} {k} {p}" for n, k, p in queries]))))
    for (n, k, parts), c in cut.items():
        assert c <= n and (c % 8 == 0 or c == n), (n, k, parts, c)
        assert (k != 0 or c == 0) and (k != parts or c == n)
    cases = set()
    for s in shards:
        world = len(s) - 1
        for parts in range(1, 5):
            for k in range(parts):
                lo = [s[r] + cut[(s[r + 1] - s[r], k, parts)] for r in range(world)]
                hi = [s[r] + cut[(s[r + 1] - s[r], k + 1, parts)] for r in range(world)]
                cases.add((tuple(lo), tuple(h - l for l, h in zip(lo, hi))))
    return sorted(cases)


def _plans(driver, cases, have_send_recv):
    lines = []
    for first, count in cases:
        pieces = " ".join(f"{f} {c}" for f, c in zip(first, count))
        lines += [f"P {rank} {len(first)} {int(have_send_recv)} {pieces}" for rank in range(len(first))]
    out = iter(driver(lines))
    plans = []
    for first, _ in cases:
        per_rank = []
        for _rank in first:
            v = [int(x) for x in next(out).split()]
            per_rank.append((bool(v[0]), [tuple(v[i:i + 4]) for i in range(1, len(v), 4)]))
        plans.append(per_rank)
    return plans


@pytest.mark.parametrize("have_send_recv", [True, False])
def test_every_rank_receives_every_other_piece_once(driver, have_send_recv):
    cases = _cases(driver)
    assert len(cases) > 500 and {len(f) for f, _ in cases} == set(range(1, 9))
    assert any(0 in c and any(c) for _, c in cases)                  # some ranks have nothing to give
    n_equal = n_exchanged = 0
    for (first, count), plans in zip(cases, _plans(driver, cases, have_send_recv)):
        W = len(first)
        what = (first, count, have_send_recv)
        if all(count[r] == count[0] and first[r] == first[0] + r * count[0] for r in range(W)):
            # equal pieces side by side in rank order: one in-place all-gather (none when they are empty), no group
            n_equal += 1
            for grouped, ops in plans:
                assert not grouped and ops == ([(ALLGATHER, -1, first[0], count[0])] if count[0] else []), what
            continue
        n_exchanged += 1
        sends, recvs = {}, {}          # (from, to) -> pieces in issue order
        bcasts = []
        for me, (grouped, ops) in enumerate(plans):
            assert grouped, what
            kinds = {op[0] for op in ops}
            assert ALLGATHER not in kinds and kinds <= ({SEND, RECV} if have_send_recv else {BCAST}), what
            got = {}
            for kind, peer, f, c in ops:
                assert 0 <= peer < W and c > 0, what
                if kind == SEND:
                    assert peer != me and (f, c) == (first[me], count[me]), what
                    sends.setdefault((me, peer), []).append((f, c))
                elif kind == RECV:
                    assert peer != me, what
                    recvs.setdefault((peer, me), []).append((f, c))
                    got.setdefault(peer, []).append((f, c))
                elif peer != me:
                    got.setdefault(peer, []).append((f, c))
            if have_send_recv:   # round k: to rank me + k, from rank me - k (a different pair of peers every round)
                rounds = [((me + k) % W, (me - k) % W) for k in range(1, W)]
                assert [op[1] for op in ops if op[0] == SEND] == [to for to, _ in rounds if count[me]], what
                assert [op[1] for op in ops if op[0] == RECV] == [fr for _, fr in rounds if count[fr]], what
            if kinds == {BCAST} or not ops:
                bcasts.append([op for op in ops if op[0] == BCAST])
            # every other rank's non-empty piece exactly once, at its place; nothing into this rank's own piece
            assert got == {q: [(first[q], count[q])] for q in range(W) if q != me and count[q]}, what
            for f, c in (x for v in got.values() for x in v):
                assert f + c <= first[me] or first[me] + count[me] <= f or not count[me], what
        # every send meets a receive of the same piece on its peer, in the same order per ordered pair
        assert sends == recvs, what
        # broadcasts are collectives: every rank issues the same ones, each root broadcasting its own piece
        if not have_send_recv:
            assert all(b == bcasts[0] for b in bcasts) and len(bcasts) == W, what
            assert bcasts[0] == [(BCAST, r, first[r], count[r]) for r in range(W) if count[r]], what
    assert n_equal > 50 and n_exchanged > 50
