"""What speed perturbation costs, per call and per training step --
  call      alacgpu_resample_ratio_rows_device alone (ctx.resample_ratio_rows_device) on [64, 1, Ls] into [64, 1, 32000], Ls the
            source frames 32000 output frames need, at 9 : 10 and 11 : 10 against alac.resample's kernel on the same rows
            (ctx.resample_device with the ratio's table: the table kernel can do those two), and at 3969 : 1600 alone, which
            no table kernel here can do.  _measure.event_ms, the ways alternating inside every repetition: median and
            p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, check=False) on 44.1 kHz files with
            speed=SpeedPerturb() and without: _measure.wall_ms, median and p10 .. p90.
With --parent DIR (a built tree of the parent commit) the parent's ratio call and the parent's speed step alternate with this
tree's: the outputs have to be equal, and this tree's median has to lie inside the parent's p10 .. p90.
One JSON document, printed and written to --out.
  python tools/bench_speed.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/speed.json]"""
import argparse
import sys

import numpy as np

from _measure import arguments, device, emit, event_ms, inside, load_parent, make_file, stats, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=30.0)
    arguments(ap, "speed.json", reps=10, parent="a built tree of the parent commit: its ratio call and its speed step alternate with this tree's")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth
    from alac.net_amd.resample import device_table, filter_width

    synth.build()
    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    parent_pkg = load_parent(args.parent) if args.parent else None

    # ---- the call alone --------------------------------------------------------------------------------------------------------
    calls = []
    B, L = 64, 32000
    parent_ctx = parent_pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) if parent_pkg else None
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        for a, b in ((9, 10), (11, 10), (3969, 1600)):
            width = filter_width(a, b)
            Ls = -(-L * a // b)
            x = torch.from_numpy(rng.uniform(-1, 1, (B, 1, Ls)).astype(np.float32)).to(dev)
            zeros = torch.zeros(B, dtype=torch.int64, device=dev)
            valid = torch.full((B,), Ls, dtype=torch.int64, device=dev)
            ratios = np.array([[a, b, width]], dtype=np.uint32)
            d_ratios = torch.from_numpy(ratios.view(np.int32)).to(dev)
            row_ratio = torch.zeros(B, dtype=torch.int32, device=dev)
            out, out_t = torch.empty((B, 1, L), dtype=torch.float32, device=dev), torch.empty((B, 1, L), dtype=torch.float32, device=dev)
            ways = {"ratio_call": lambda: ctx.resample_ratio_rows_device(x, B, 1, Ls, zeros, valid, zeros, L, ratios, d_ratios, row_ratio,
                                                                         False, out, stream=stream.cuda_stream)}
            table = b * (2 * width + 1) <= 16384
            if table:
                _, _, _, d_d0, d_w = device_table(a, b, dev)
                ways["table_call"] = lambda: ctx.resample_device(x, B, 1, Ls, zeros, valid, zeros, L, a, b, width, d_d0, d_w, False, out_t,
                                                                 stream=stream.cuda_stream)
            if parent_pkg is not None:
                theirs = torch.empty((B, 1, L), dtype=torch.float32, device=dev)
                ways["parent_ratio_call"] = lambda: parent_ctx.resample_ratio_rows_device(x, B, 1, Ls, zeros, valid, zeros, L, ratios, d_ratios,
                                                                                         row_ratio, False, theirs, stream=stream.cuda_stream)
            for fn in ways.values():
                fn()
            torch.cuda.synchronize()
            assert parent_pkg is None or torch.equal(out, theirs), "the ratio call's output differs from the parent's"
            ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=True)
            doc = {"ratio": [a, b], "width": width, "src_shape": [B, 1, Ls], "out_shape": [B, 1, L],
                   "ms_per_call_events_around_reps_calls": {m: stats(v) for m, v in ms.items()}}
            if parent_pkg is not None:
                doc["ratio_call_inside_parent_p10_p90"] = inside(doc["ms_per_call_events_around_reps_calls"]["parent_ratio_call"],
                                                                 doc["ms_per_call_events_around_reps_calls"]["ratio_call"])
            if table:
                doc["max_abs_difference_to_table_call"] = float((out - out_t).abs().max())
                r, t = doc["ms_per_call_events_around_reps_calls"]["ratio_call"], doc["ms_per_call_events_around_reps_calls"]["table_call"]
                doc["ratio_call_median_over_table_call_median"] = r["median"] / t["median"]
            calls.append(doc)

    # ---- the step --------------------------------------------------------------------------------------------------------------
    rate, R = 44100, 16000
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    corpus = pkg.Corpus([distinct[f % 2] for f in range(args.files)])
    kw = dict(sample_rate=R, mono=True, check=False)
    sp = pkg.SpeedPerturb()
    ways = {"speed": lambda i: corpus.random_crops(B, L, speed=sp, **kw)[0], "without": lambda i: corpus.random_crops(B, L, **kw)[0]}
    if parent_pkg is not None:
        parent_ctx.close()
        parent, psp = parent_pkg.Corpus([distinct[f % 2] for f in range(args.files)]), parent_pkg.SpeedPerturb()
        ways["parent_speed"] = lambda i: parent.random_crops(B, L, speed=psp, **kw)[0]
        ways["parent_without"] = lambda i: parent.random_crops(B, L, **kw)[0]
        for seed in (3, 4):      # one seeded generator on both sides: the same draws, and the same crops of them
            g = [torch.Generator(device=dev).manual_seed(seed) for _ in range(2)]
            for mine, theirs in ((corpus.random_crops(B, L, speed=sp, generator=g[0], **kw), parent.random_crops(B, L, speed=psp, generator=g[1], **kw)),
                                 (corpus.random_crops(B, L, generator=g[0], **kw), parent.random_crops(B, L, generator=g[1], **kw))):
                assert all(torch.equal(x, y) for x, y in zip(mine, theirs)), "random_crops differs from the parent's"
    wall = wall_ms(torch, ways, args.steps, args.warmup)
    corpus.close()
    if parent_pkg is not None:
        parent.close()
    step = {"step": "random_crops(64, 32000, sample_rate=16000, mono=True, check=False) on 44.1 kHz stereo files",
            "speed": "speed=SpeedPerturb(): 0.9 / 1.0 / 1.1, that is 3969 : 1600, 441 : 160 (the table kernel) and 4851 : 1600",
            "wall_ms": {m: stats(v) for m, v in wall.items()}}
    if parent_pkg is not None:
        step.update({f"{m}_inside_parent_p10_p90": inside(step["wall_ms"]["parent_" + m], step["wall_ms"][m]) for m in ("speed", "without")})
    shown = [a for i, a in enumerate(sys.argv[1:], 1) if a not in ("--out", "--parent") and sys.argv[i - 1] not in ("--out", "--parent")]     # (where it was written, and where the parent's tree lay, say nothing)
    doc = {"command": " ".join(["python tools/bench_speed.py"] + shown), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "calls": calls, "step": step}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
