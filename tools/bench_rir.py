"""What the simulated room responses cost --
  call      simulate_rir on 64 rows at 16 kHz, K = 8000, taps 81, rooms drawn from ShoeboxRooms.kaldi("small" | "medium" |
            "large") with a seeded generator, and the same rows by a torch composition: the candidate box enumerated as
            tensors in chunks, float64 sqrt, the order and reach tests, the window and the sinc over the 81 offsets,
            index_add_ into the row.  _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
            The composition is timed on --compose-rows rows (default 4) and scaled to 64: it takes seconds a row.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, reverb=..., check=False) with a Reverb over rooms
            (the default ShoeboxRooms, max_seconds 0.5), with a Reverb over a corpus of responses and without reverb=
            (_measure.wall_ms, the ways in turn), and with --parent DIR (a built tree of the parent commit) the corpus-Reverb
            step by this tree's package and by the parent's, in turn: "unchanged_step_overlaps_parent" is whether their
            p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_rir.py [--steps 20] [--warmup 3] [--parent DIR] [--out profiles/rir.json]"""
import argparse
import math
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms

B, K, RATE, T, W = 64, 8000, 16000, 32000, 81


def composed(torch, pkg, geometry, beta, out):
    """The torch composition of the same rows: every candidate of the box as tensors, 2^18 at a time"""
    H, scale = W // 2, RATE / 343.0
    m = torch.arange(-H, H + 1, device=geometry.device)
    G, Bt = geometry.cpu().numpy(), beta.double()
    out.zero_()
    for b in range(geometry.shape[0]):
        N = pkg.rir.candidate_box(G[b], scale, K, H, -1)
        if N is None:
            continue
        L, s, r = geometry[b, 0:3], geometry[b, 3:6], geometry[b, 6:9]
        sizes = [2 * n + 1 for n in N] + [8]
        total = sizes[0] * sizes[1] * sizes[2] * 8
        row = torch.zeros(K, dtype=torch.float64, device=geometry.device)
        for lo in range(0, total, 1 << 18):
            j = torch.arange(lo, min(lo + (1 << 18), total), device=geometry.device)
            pi, j = j % 8, j // 8
            nz, j = j % sizes[2] - N[2], j // sizes[2]
            ny, nx = j % sizes[1] - N[1], j // sizes[1] - N[0]
            n = torch.stack([nx, ny, nz], dim=1)
            p = torch.stack([pi >> 2, (pi >> 1) & 1, pi & 1], dim=1)
            x = (1 - 2 * p) * s + 2 * n * L - r
            d = x.pow(2).sum(dim=1).sqrt()
            tau = d * scale
            keep = tau < K + H
            n, p, d, tau = n[keep], p[keep], d[keep], tau[keep]
            e = torch.stack([(n - p).abs(), n.abs()], dim=2).reshape(-1, 6)
            A = (Bt[b][None, :] ** e).prod(dim=1) / (4 * math.pi * d)
            k = torch.floor(tau + 0.5).long()[:, None] + m[None, :]
            t = k - tau[:, None]
            v = A[:, None] * 0.5 * (1 + torch.cos(2 * math.pi * t / W)) * torch.sinc(t) * (t.abs() < W / 2)
            ok = (k >= 0) & (k < K)
            row.index_add_(0, k[ok], v[ok])
        out[b, 0] = row.float()
    return out


def step_of(corpus, torch, reverb):
    g = torch.Generator().manual_seed(3)
    kw = {} if reverb is None else dict(reverb=reverb)
    return lambda i: corpus.random_crops(B, T, generator=g, sample_rate=RATE, mono=True, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "rir.json", reps=1, parent="a built tree of the parent commit: the unchanged corpus-Reverb step is timed on both")
    ap.add_argument("--compose-rows", type=int, default=4)
    ap.add_argument("--compose-steps", type=int, default=3)
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "rows": B, "frames": K, "rate": RATE, "taps": W,
           "ms_per_call": {}, "unmeasured": ["counters (rocprofv3 --pmc): how close the kernel comes to the VALU issue rate",
                                             "kernel time by rocprofv3 --kernel-trace", "rates other than 16 kHz", "max_order"]}
    for size in ("small", "medium", "large"):
        rooms = pkg.ShoeboxRooms.kaldi(size)
        geometry, beta = rooms.draw(B, generator=torch.Generator().manual_seed(1), device=dev)
        out = torch.empty((B, 1, K), dtype=torch.float32, device=dev)
        ours = event_ms(torch, stream, {"simulate_rir": lambda: pkg.simulate_rir(geometry, beta, RATE, K, out=out)}, args.steps,
                        args.warmup, args.reps, alternate=False)
        boxes = [pkg.rir.candidate_box(g, RATE / 343.0, K, W // 2, -1) for g in geometry.cpu().numpy()]
        sizes = [0 if n is None else 8 * (2 * n[0] + 1) * (2 * n[1] + 1) * (2 * n[2] + 1) for n in boxes]
        entry = {"simulate_rir": stats(ours["simulate_rir"]), "rows_refused": sizes.count(0),
                 "candidates_a_row_median_and_max": [int(np.median(sizes)), int(max(sizes))]}
        R = args.compose_rows
        if R:
            ref = torch.empty((R, 1, K), dtype=torch.float32, device=dev)
            theirs = event_ms(torch, stream, {"torch": lambda: composed(torch, pkg, geometry[:R], beta[:R], ref)}, args.compose_steps, 1, 1,
                              alternate=False)
            entry["torch_composition_on_%d_rows" % R] = stats(theirs["torch"])
            entry["torch_composition_scaled_to_64_rows_multiple_of_simulate_rir"] = round(
                stats(theirs["torch"])["median"] * B / R / entry["simulate_rir"]["median"], 1)
            entry["largest_difference_from_the_composition"] = float((out[:R] - ref).abs().max())
        doc["ms_per_call"][size] = entry
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths, responses = [], []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as fh:
                fh.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=44100))
            responses.append(os.path.join(tmp, f"r{i}.m4a"))
            with open(responses[-1], "wb") as fh:
                fh.write(make_file(synth, 20000 + 321 * i, 40 + i, rate=16000))
        with pkg.Corpus(paths) as corpus, pkg.Corpus(responses) as rirs:
            rooms = pkg.Reverb(pkg.ShoeboxRooms(), max_seconds=0.5)
            recorded = pkg.Reverb(rirs, max_seconds=0.5)
            ms = wall_ms(torch, {"step_rooms": step_of(corpus, torch, rooms), "step_response_corpus": step_of(corpus, torch, recorded),
                                 "step_pcm": step_of(corpus, torch, None)}, args.steps, args.warmup)
            doc["step_wall_ms"] = {k: stats(v) for k, v in ms.items()}
            doc["unchanged_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs, parent.Corpus(responses) as their_rirs:
                    old = parent.Reverb(their_rirs, max_seconds=0.5)
                    ms = wall_ms(torch, {"this": step_of(corpus, torch, recorded), "parent": step_of(theirs, torch, old)}, args.steps,
                                 args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["unchanged_step_wall_ms"] = both
                    doc["unchanged_step_overlaps_parent"] = overlap(both["this"], both["parent"])
    emit(doc, args.out)


if __name__ == "__main__":
    main()
