"""What a resident corpus is worth per training step: B random crops of L frames out of synthetic M4A files (stereo 16-bit,
4096-frame packets, 60 s each), three ways on the same crops --
  (a) load_batch  load_batch(file bytes of every crop, frame_offsets=, max_frames=): demux, plan, upload and a context per call
  (b) corpus_host corpus.crops with host index arrays and check=True (two small uploads, one small read)
  (c) corpus_dev  corpus.crops with device index tensors and check=False (nothing but the enqueue)
Per (B, L): the wall time of a step (_measure.wall_ms, median), the planning kernel's time (HIP events around --plan-reps
back-to-back launches, divided by them, median) and the padding share 1 - packets / (B * K).  The three are checked equal
once.  One JSON line.
  python tools/bench_corpus.py [--files 32] [--seconds 60] [--steps 30] [--warmup 5]
With --hbm-bytes N a fourth way on a second corpus, Corpus(files, hbm_bytes=N):
  (d) corpus_tiered  as (c), the packets of the step staged from page-locked host memory (alacgpu_stage_packets_device)
and per shape the staging capacity and the bytes a step staged.
Kernel times of the decode pair: run one way alone under the profiler's kernel trace, e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_corpus.py --only corpus_dev --shape 64x88200"""
import argparse
import json

import numpy as np

from _measure import device, make_file, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--distinct", type=int, default=2, help="distinct files behind the sources (the bytes are shared)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plan-reps", type=int, default=20)
    ap.add_argument("--shape", action="append", help="BxL, repeatable (default 64x88200 and 256x44100)")
    ap.add_argument("--only", choices=["load_batch", "corpus_host", "corpus_dev", "corpus_tiered"], help="run this way alone (for a kernel trace)")
    ap.add_argument("--hbm-bytes", type=int, help="also measure a corpus that keeps only this many packet bytes in HBM (way corpus_tiered)")
    args = ap.parse_args()
    if args.only == "corpus_tiered" and args.hbm_bytes is None:
        ap.error("--only corpus_tiered needs --hbm-bytes")
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    dev, stream = device(torch)
    T = int(args.seconds * 44100)
    distinct = [make_file(synth, T, 11 + k) for k in range(args.distinct)]
    blobs = [distinct[f % len(distinct)] for f in range(args.files)]
    shapes = [tuple(int(x) for x in s.split("x")) for s in (args.shape or ["64x88200", "256x44100"])]
    corpus = pkg.Corpus(blobs)
    tiered = pkg.Corpus(blobs, hbm_bytes=args.hbm_bytes) if args.hbm_bytes is not None else None
    results = []
    for B, L in shapes:
        rng = np.random.default_rng(B + L)
        draws = [(rng.integers(0, args.files, B).astype(np.int64), rng.integers(0, T - L + 1, B).astype(np.int64))
                 for _ in range(args.steps + args.warmup)]
        on_device = [(torch.from_numpy(f).to(dev), torch.from_numpy(o).to(dev)) for f, o in draws]

        def load_batch(i):
            f, o = draws[i]
            return pkg.load_batch([blobs[k] for k in f], frame_offsets=o, max_frames=L)[0]

        def corpus_host(i):
            return corpus.crops(draws[i][0], draws[i][1], L)[0]

        def corpus_dev(i):
            return corpus.crops(on_device[i][0], on_device[i][1], L, check=False)[0]

        def corpus_tiered(i):
            return tiered.crops(on_device[i][0], on_device[i][1], L, check=False)[0]

        modes = {"load_batch": load_batch, "corpus_host": corpus_host, "corpus_dev": corpus_dev}
        if tiered is not None:
            modes["corpus_tiered"] = corpus_tiered
        if args.only:
            modes = {args.only: modes[args.only]}
        else:
            outs = [fn(0) for fn in modes.values()]
            assert all(torch.equal(outs[0], x) for x in outs[1:]), "the three ways differ" if tiered is None else "the four ways differ"
            del outs
        wall = wall_ms(torch, modes, args.steps, args.warmup)
        med = lambda v: round(float(np.median(v)), 4)
        r = {"crops": B, "crop_frames": L, "wall_ms": {m: med(v) for m, v in wall.items()}}
        if not args.only:
            # the planner alone, and the padding share of the plan it writes
            K = corpus.entries_per_crop(L)
            corpus.crops(on_device[0][0], on_device[0][1], L, check=False)
            valid = corpus.last_status()[1]
            pl, lengths = corpus._plan, torch.empty(B, dtype=torch.int64, device=dev)

            f, o = on_device[0][0].to(torch.int32), on_device[0][1]

            def plan():
                rc = pkg.lib().alacgpu_plan_crops_device(
                    corpus._gpu._ctx, pkg._dp(corpus._pkt_offset), pkg._dp(corpus._pkt_size), pkg._dp(corpus._pkt_end),
                    pkg._dp(corpus._file_first), pkg._dp(corpus._file_cfg), corpus.num_files, pkg._dp(f), pkg._dp(o), B, L, K,
                    2 * L, pkg._dp(pl["offsets"]), pkg._dp(pl["sizes"]), pkg._dp(pl["cfg_idx"]), pkg._dp(pl["dst_first"]),
                    pkg._dp(pl["dst_frames"]), pkg._dp(pl["src_skip"]), pkg._dp(lengths), pkg._VP(stream.cuda_stream))
                assert rc == 0, rc

            ms = []                                         # (no synchronize in front of the events: not _measure.event_ms)
            for rep in range(args.steps + args.warmup):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.plan_reps):
                    plan()
                e1.record(stream)
                e1.synchronize()
                if rep >= args.warmup:
                    ms.append(e0.elapsed_time(e1) / args.plan_reps)
            r.update(entries_per_crop=K, packets=int(valid.sum()), padding_share=round(1.0 - float(valid.sum()) / (B * K), 4),
                     plan_kernel_ms=med(ms), speedup_dev_vs_load_batch=round(med(wall["load_batch"]) / med(wall["corpus_dev"]), 2))
        if tiered is not None and tiered.tier_bytes[1]:
            tiered.crops(on_device[0][0], on_device[0][1], L, check=False)
            r.update(stage_capacity_bytes=B * tiered.stage_bytes_per_crop(L), staged_bytes=int(tiered.last_staged_bytes()[0]))
        results.append(r)
    corpus.close()
    head = {"files": args.files, "seconds": args.seconds, "steps": args.steps, "warmup": args.warmup,
            "blob_mb": round(corpus._blob_bytes / 1e6, 1)}
    if tiered is not None:
        head.update(hbm_bytes=args.hbm_bytes, tier_bytes=list(tiered.tier_bytes))
        tiered.close()
    print(json.dumps({**head, "results": results}), flush=True)


if __name__ == "__main__":
    main()
