"""What the YIN stage costs --
  call      yin(x, Yin(16000), lengths, out=track) on [64, 1, 32000] with random lengths in 16000 .. 32000, against the same
            thing composed in torch on the same tensor: zero padding and unfold into frames, the difference function as
            librosa builds it (the autocorrelation by rfft / irfft plus cumulative energies), cumsum, the compares and gather
            for the threshold search, the descent left out (it only makes the composition cheaper than the real thing).
            _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=LogMel(16000), check=False) with and
            without f0=Yin.like(spec) (_measure.wall_ms, the ways in turn), and with --parent DIR (a built tree of the parent
            commit) the step without f0= by this tree's package and by the parent's, in turn:
            "unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_yin.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/yin.json]"""
import argparse
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms


def step_of(pkg, corpus, torch, **kw):
    spec = pkg.LogMel(16000)
    g = torch.Generator().manual_seed(3)
    if kw.pop("f0", False):
        kw["f0"] = pkg.Yin.like(spec)
    return lambda i: corpus.random_crops(64, 32000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "yin.json", reps=10, parent="a built tree of the parent commit: the unchanged step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    B, T, rate = 64, 32000, 16000
    spec = pkg.Yin(rate)
    t = np.arange(T) / rate
    f = rng.uniform(80.0, 300.0, (B, 1, 1))
    x = torch.from_numpy((0.4 * np.sin(2 * np.pi * f * t) + 0.05 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    lengths = torch.from_numpy(rng.integers(T // 2, T + 1, B)).to(dev)
    track = torch.empty((B, 1, 2, spec.frames(T)), dtype=torch.float32, device=dev)
    W, hop, lo, hi, n = spec.win_length, spec.hop_length, spec.tau_min, spec.tau_max, 2048
    mask = torch.arange(T, device=dev)[None, :] < lengths[:, None]
    lag = torch.arange(1, hi + 1, device=dev, dtype=torch.float32)

    def composed():
        xp = torch.nn.functional.pad(torch.where(mask, x[:, 0], 0.0), (-spec.first, spec.span))
        fr = xp.unfold(1, spec.span, hop)[:, :spec.frames(T)]                              # [B, T', span]
        a = torch.fft.rfft(fr, n)
        b = torch.fft.rfft(fr[..., :W].flip(-1), n)
        acf = torch.fft.irfft(a * b, n)[..., W - 1:W + hi]                                 # r[tau], tau = 0 .. hi
        e = torch.nn.functional.pad(fr * fr, (1, 0)).cumsum(-1)
        energy = e[..., W:W + hi + 1] - e[..., 0:hi + 1]
        d = energy[..., :1] + energy - 2.0 * acf
        dp = d[..., 1:] * lag / d[..., 1:].cumsum(-1).clamp_min(1e-30)
        cand = dp[..., lo - 1:hi - 1]
        below = cand < spec.threshold
        first = torch.where(below.any(-1), below.float().argmax(-1), cand.argmin(-1))
        ap_ = cand.gather(-1, first[..., None])[..., 0]
        track[:, 0, 0] = rate / (first + lo).float()
        track[:, 0, 1] = ap_

    ways = {"yin": lambda: pkg.yin(x, spec, lengths, out=track), "torch_composed": composed}
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False)
    calls = {k: stats(v) for k, v in ms.items()}
    pairs = int(spec.lengths(lengths.cpu().numpy()).sum()) * W * (hi + 1)
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "spec": repr(spec), "ms_per_call_events_around_reps_calls": calls,
           "composed_multiple_of_yin": round(calls["torch_composed"]["median"] / calls["yin"]["median"], 2),
           "subtract_fma_pairs_per_call": pairs,
           "pairs_per_second": round(pairs / (calls["yin"]["median"] * 1e-3))}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as fh:
                fh.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_f0": step_of(pkg, corpus, torch, f0=True)}, args.steps, args.warmup)
            both = {k: stats(v) for k, v in ms.items()}
            doc["step_wall_ms"] = both
            doc["step_f0_multiple_of_step"] = round(both["step_f0"]["median"] / both["step"]["median"], 3)
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
