"""What the level stage costs --
  call      level(x, spec, 16000, lengths, out=x) in place on [64, 1, 32000] with random lengths, in the three modes, each against
            the same thing composed: peak and rms from torch (amax / a masked mean square, mul), lufs from the project's own
            pieces -- alac.biquad with the two K-weighting sections out of place, unfold over the hops, means, compares, mul
            (torch has no IIR) --, and against alac.biquad with those 2 sections in place, the call the measure launch is
            expected near.  x is restored from a copy in front of every repetition, outside the events.
            _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=KaldiFbank(16000), check=False) with and
            without level=Level.lufs() (_measure.wall_ms, the ways in turn), and with --parent DIR (a built tree of the parent
            commit) the step without level= by this tree's package and by the parent's, in turn:
            "unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_level.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/level.json]"""
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
    arguments(ap, "level.json", reps=10, parent="a built tree of the parent commit: the unchanged step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    B, T, rate, hop = 64, 32000, 16000, 1600
    x = torch.from_numpy((0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    lengths = torch.from_numpy(rng.integers(T // 2, T + 1, B)).to(dev)
    x0 = x.clone()
    mask = (torch.arange(T, device=dev)[None, :] < lengths[:, None])[:, None, :]
    kw = torch.from_numpy(pkg.kweight(rate)).to(dev)
    blocks = (torch.arange(T // hop - 3, device=dev)[None, :] < (lengths // hop - 3)[:, None])

    def torch_peak():
        g = 1.0 / torch.where(mask, x.abs(), 0.0).amax(dim=(1, 2), keepdim=True)
        x.mul_(torch.where(mask, g, 1.0))

    def torch_rms():
        e = torch.where(mask, x.double() ** 2, 0.0).sum(dim=(1, 2), keepdim=True) / lengths[:, None, None]
        x.mul_(torch.where(mask, torch.sqrt(10.0 ** -2.5 / e).float(), 1.0))

    def composed_lufs():
        w = pkg.biquad(x, kw, lengths)                                        # (out of place: x is needed again)
        z = torch.where(mask, w.double() ** 2, 0.0)[:, 0].unfold(1, 4 * hop, hop).mean(dim=2)
        above = blocks & (z > 10.0 ** -6.9309)
        m1 = torch.where(above, z, 0.0).sum(dim=1, keepdim=True) / above.sum(dim=1, keepdim=True)
        both = above & (z > 0.1 * m1)
        e = torch.where(both, z, 0.0).sum(dim=1) / both.sum(dim=1)
        x.mul_(torch.where(mask, torch.sqrt(10.0 ** -2.2309 / e).float()[:, None, None], 1.0))

    ways = {"level_peak": lambda: pkg.level(x, pkg.Level.peak(1.0), rate, lengths, out=x), "torch_peak": torch_peak,
            "level_rms": lambda: pkg.level(x, pkg.Level.rms(-25.0), rate, lengths, out=x), "torch_rms": torch_rms,
            "level_lufs": lambda: pkg.level(x, pkg.Level.lufs(-23.0), rate, lengths, out=x), "composed_lufs": composed_lufs,
            "loudness": lambda: pkg.loudness(x, rate, lengths), "biquad_S2": lambda: pkg.biquad(x, kw, lengths, out=x)}
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False, before=dict.fromkeys(ways, lambda: x.copy_(x0)))
    calls = {k: stats(v) for k, v in ms.items()}
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "ms_per_call_events_around_reps_calls": calls,
           "level_lufs_multiple_of_biquad_S2": round(calls["level_lufs"]["median"] / calls["biquad_S2"]["median"], 2),
           "composed_multiples_of_level": {m: round(calls[c]["median"] / calls[f"level_{m}"]["median"], 2)
                                           for m, c in (("peak", "torch_peak"), ("rms", "torch_rms"), ("lufs", "composed_lufs"))}}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as f:
                f.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_lufs": step_of(pkg, corpus, torch, level=pkg.Level.lufs())},
                         args.steps, args.warmup)
            both = {k: stats(v) for k, v in ms.items()}
            doc["step_wall_ms"] = both
            doc["step_lufs_multiple_of_step"] = round(both["step_lufs"]["median"] / both["step"]["median"], 3)
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
