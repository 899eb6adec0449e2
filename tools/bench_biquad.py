"""What the biquad stage costs --
  call      biquad(x, coeffs, lengths, gain, out=x) in place on [64, 1, 32000] with random lengths and S = 1, 4 and 8 sections,
            against torch.mul(x, 1.0, out=x) on the same tensor: one read and one write, the floor of an in-place stage.
            x is restored from a copy in front of every repetition, outside the events, so that no call filters silence.
            _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=KaldiFbank(16000), check=False) with and
            without effects=Effects.telephone() (_measure.wall_ms, the ways in turn), and with --parent DIR (a built tree of the
            parent commit) the step without effects= by this tree's package and by the parent's, in turn:
            "unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_biquad.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/biquad.json]"""
import argparse
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms


def step_of(pkg, corpus, torch, **kw):
    spec = pkg.KaldiFbank(16000)
    g = torch.Generator().manual_seed(3)
    return lambda i: corpus.random_crops(64, 32000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "biquad.json", reps=10, parent="a built tree of the parent commit: the unchanged step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    B, T = 64, 32000
    x = torch.from_numpy((0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    lengths = torch.from_numpy(rng.integers(T // 2, T + 1, B)).to(dev)
    gain = torch.from_numpy(rng.uniform(0.5, 1.0, B)).to(dev)
    fx = pkg.Effects(tuple(pkg.RandomBiquad("peaking", (200.0, 6000.0), q=(0.5, 2.0), gain_db=(-3.0, 0.0)) for _ in range(8)))
    coeffs = fx.draw(B, 16000, generator=torch.Generator().manual_seed(2), device=dev)[0]
    x0 = x.clone()
    ways = {"mul": lambda: torch.mul(x, 1.0, out=x)}
    for S in (1, 4, 8):
        ways[f"biquad_S{S}"] = lambda q=coeffs[:, :S].contiguous(): pkg.biquad(x, q, lengths, gain, out=x)
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False, before=dict.fromkeys(ways, lambda: x.copy_(x0)))
    calls = {k: stats(v) for k, v in ms.items()}
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "ms_per_call_events_around_reps_calls": calls,
           "multiples_of_mul": {k: round(v["median"] / calls["mul"]["median"], 2) for k, v in calls.items() if k != "mul"}}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as f:
                f.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_telephone": step_of(pkg, corpus, torch, effects=pkg.Effects.telephone())},
                         args.steps, args.warmup)
            both = {k: stats(v) for k, v in ms.items()}
            doc["step_wall_ms"] = both
            doc["step_telephone_multiple_of_step"] = round(both["step_telephone"]["median"] / both["step"]["median"], 3)
            doc["unchanged_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs:
                    ms = wall_ms(torch, {"this": step_of(pkg, corpus, torch), "parent": step_of(parent, theirs, torch)}, args.steps, args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["unchanged_step_wall_ms"] = both
                    doc["unchanged_step_overlaps_parent"] = overlap(both["this"], both["parent"])
    emit(doc, args.out)


if __name__ == "__main__":
    main()
