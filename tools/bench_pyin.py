"""What the pYIN stage costs --
  call      pyin(x, PYin(16000), lengths, out=track) on [64, 1, 32000] with random lengths in 16000 .. 32000, its two launches
            apart (pyin_observation; pyin_decode on those observations) and yin(x, Yin(16000), lengths) on the same tensor.
            _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
  long      pyin_decode on [16, 1, 3001 frames] (480000 samples a row) of observations: the recursion with a walk back of 3001
            dependent loads a line.
  torch     the recursion composed in torch is a Python loop over the frames: a max over the banded transition matrix per frame
            and half, on 2 rows of 201 frames, the walk back left out; "torch_scaled_to_64_rows" is that time times 32 -- a
            scaling, not a measurement (a loop of launches does not get 32 times slower with 32 times the rows).
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=LogMel(16000), check=False) without f0=, with
            f0=Yin.like(spec) and with f0=PYin.like(spec) (_measure.wall_ms, the ways in turn), and with --parent DIR (a built
            tree of the parent commit) the step with f0=Yin.like(spec) by this tree's package and by the parent's, in turn:
            "yin_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out; the counts tests/test_pyin_spec.py recorded there are kept.
  python tools/bench_pyin.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/pyin.json]"""
import argparse
import json
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms

KEEP = "noise_200hz_9db"


def step_of(pkg, corpus, torch, f0=None):
    spec = pkg.LogMel(16000)
    g = torch.Generator().manual_seed(3)
    kw = {} if f0 is None else {"f0": getattr(pkg, f0).like(spec)}
    return lambda i: corpus.random_crops(64, 32000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "pyin.json", reps=10, parent="a built tree of the parent commit: the step with f0=Yin is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    B, T, rate = 64, 32000, 16000
    spec, plain = pkg.PYin(rate), pkg.Yin(rate)
    t = np.arange(T) / rate
    f = rng.uniform(80.0, 300.0, (B, 1, 1))
    x = torch.from_numpy((0.4 * np.sin(2 * np.pi * f * t) + 0.05 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    lengths = torch.from_numpy(rng.integers(T // 2, T + 1, B)).to(dev)
    n, F = spec.n_bins, int(spec.frames(T))
    track = torch.empty((B, 1, 3, F), dtype=torch.float32, device=dev)
    track2 = torch.empty((B, 1, 2, F), dtype=torch.float32, device=dev)
    ov, ou, _ = pkg.pyin_observation(x, spec, lengths)
    counts = spec.lengths(lengths)
    long_v = ov[:16, :, :1].expand(16, 1, 3001, n).contiguous()
    long_v += torch.from_numpy(rng.uniform(-1.0, 0.0, (16, 1, 3001, n)).astype(np.float32)).to(dev)
    long_u = torch.full((16, 1, 3001), -9.0, dtype=torch.float32, device=dev)
    tab = {k: torch.from_numpy(v).to(dev) for k, v in spec.tables().items()}
    at = torch.arange(n, device=dev)
    off = (at[None, :] - at[:, None]).abs()
    logT = torch.where(off <= spec.h, tab["lt"][off.clamp_max(spec.band)] - tab["lz"][:, None], torch.full((), -float("inf"), device=dev))

    def composed():
        v, u = ov[:2, 0], ou[:2, 0]
        obs = torch.cat([v, u[..., None].expand(2, F, n)], dim=-1)
        delta = tab["lstart"] + obs[:, 0]
        for k in range(1, F):
            m = (delta.view(2, 2, n, 1) + logT).max(dim=2)[0]                                 # [rows, half, target]
            stay, switch = m + tab["ls"][0], m.flip(1) + tab["ls"][1]
            delta = obs[:, k] + torch.maximum(stay, switch).reshape(2, 2 * n)
        return delta.argmax(-1)

    ways = {"pyin": lambda: pkg.pyin(x, spec, lengths, out=track), "observation": lambda: pkg.pyin_observation(x, spec, lengths),
            "decode": lambda: pkg.pyin_decode(ov, ou, spec, counts), "yin": lambda: pkg.yin(x, plain, lengths, out=track2),
            "decode_16_lines_of_3001_frames": lambda: pkg.pyin_decode(long_v, long_u, spec)}
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False)
    calls = {k: stats(v) for k, v in ms.items()}
    ms = event_ms(torch, stream, {"torch_recursion_2_rows": composed}, max(args.steps // 20, 3), 2, 1, alternate=False)
    calls["torch_recursion_2_rows"] = stats(ms["torch_recursion_2_rows"])
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "spec": repr(spec), "frames": F, "n_bins": n, "band": spec.band, "ms_per_call_events_around_reps_calls": calls,
           "pyin_multiple_of_yin": round(calls["pyin"]["median"] / calls["yin"]["median"], 2),
           "torch_scaled_to_64_rows": round(32 * calls["torch_recursion_2_rows"]["median"], 1),
           "unmeasured": ["the two kernels under a profiler's counters", "the walk back apart from the recursion"]}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as fh:
                fh.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_yin": step_of(pkg, corpus, torch, "Yin"),
                                 "step_pyin": step_of(pkg, corpus, torch, "PYin")}, args.steps, args.warmup)
            both = {k: stats(v) for k, v in ms.items()}
            doc["step_wall_ms"] = both
            doc["step_pyin_multiple_of_step"] = round(both["step_pyin"]["median"] / both["step"]["median"], 3)
            doc["yin_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs:
                    ms = wall_ms(torch, {"this": step_of(pkg, corpus, torch, "Yin"), "parent": step_of(parent, theirs, torch, "Yin")},
                                 args.steps, args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["yin_step_wall_ms"] = both
                    doc["yin_step_overlaps_parent"] = overlap(both["this"], both["parent"])
    if os.path.exists(args.out):
        try:
            old = json.load(open(args.out))
            if KEEP in old:
                doc[KEEP] = old[KEEP]
        except ValueError:
            pass
    emit(doc, args.out)


if __name__ == "__main__":
    main()
