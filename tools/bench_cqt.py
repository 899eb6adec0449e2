"""What the constant-Q stage costs --
  call      cqt(x, ConstantQ(22050)) on [64, 1, 44100], against the torch composition on the same tensor (nnAudio's
            CQT1992v2 form): F.conv1d of the zero-padded row with the [2 * n_bins, 1, N_0] dense kernels -- every kernel
            zero-padded to the longest, centred -- at stride hop, then squares, sum, sqrt.  _measure.event_ms, one way after
            the other: median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 44100, sample_rate=22050, mono=True, features=..., check=False) with a ConstantQ(22050),
            with a LogMel(22050, 2048, 512, 128) and with no features (_measure.wall_ms, the ways in turn), and with --parent
            DIR (a built tree of the parent commit) the LogMel step by this tree's package and by the parent's, in turn:
            "unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_cqt.py [--steps 100] [--warmup 10] [--parent DIR] [--out profiles/cqt.json]"""
import argparse
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms

B, T, RATE = 64, 44100, 22050


def step_of(pkg, corpus, torch, features):
    g = torch.Generator().manual_seed(3)
    kw = {} if features is None else dict(features=features)
    return lambda i: corpus.random_crops(B, T, generator=g, sample_rate=RATE, mono=True, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "cqt.json", reps=5, parent="a built tree of the parent commit: the unchanged LogMel step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    spec = pkg.ConstantQ(RATE)
    x = torch.from_numpy((0.3 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    N = pkg.cqt_lengths(spec)
    N0, c = int(N[0]), N // 2
    dense = np.zeros((2 * spec.n_bins, 1, N0), dtype=np.float32)
    for k in range(spec.n_bins):
        at = int(c[0] - c[k])
        dense[k, 0, at:at + N[k]], dense[spec.n_bins + k, 0, at:at + N[k]] = spec.kernel(k)
    dense = torch.from_numpy(dense).to(dev)
    F = torch.nn.functional

    def composed():
        y = F.conv1d(F.pad(x, (int(c[0]), N0 - int(c[0]))), dense, stride=spec.hop_length)[..., :spec.frames(T)]
        return (y[:, :spec.n_bins] ** 2 + y[:, spec.n_bins:] ** 2).sqrt()

    ours = pkg.cqt(x, spec)[:, 0]
    worst = float((ours - composed()).abs().max())
    ways = {"cqt": lambda: pkg.cqt(x, spec), "torch_conv1d_dense": composed}
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False)
    calls = {k: stats(v) for k, v in ms.items()}
    total, rows = pkg.cqt_work(spec)
    frames = B * int(spec.frames(T))
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "spec": repr(spec), "ms_per_call_events_around_reps_calls": calls,
           "dense_multiple_of_cqt": round(calls["torch_conv1d_dense"]["median"] / calls["cqt"]["median"], 2),
           "largest_difference_from_the_composition": worst,
           "complex_multiply_add_rows_per_frame": {"contained": total, "issued": rows, "dense_at_N0": N0 * spec.n_bins},
           "issued_real_fma_per_second": round(2 * rows * frames / (calls["cqt"]["median"] * 1e-3)),
           "unmeasured": ["counters (rocprofv3 --pmc): where the slowest wave waits", "rates other than 22 050 Hz",
                          "36 bins an octave", "the second path (a span that holds a NaN)"]}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as fh:
                fh.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=44100))
        mel = lambda p: p.LogMel(RATE, 2048, 512, 128)
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step_cqt": step_of(pkg, corpus, torch, spec), "step_logmel": step_of(pkg, corpus, torch, mel(pkg)),
                                 "step_pcm": step_of(pkg, corpus, torch, None)}, args.steps, args.warmup)
            doc["step_wall_ms"] = {k: stats(v) for k, v in ms.items()}
            doc["unchanged_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs:
                    ms = wall_ms(torch, {"this": step_of(pkg, corpus, torch, mel(pkg)), "parent": step_of(parent, theirs, torch, mel(parent))},
                                 args.steps, args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["unchanged_step_wall_ms"] = both
                    doc["unchanged_step_overlaps_parent"] = overlap(both["this"], both["parent"])
    emit(doc, args.out)


if __name__ == "__main__":
    main()
