"""What per-channel energy normalisation costs next to what a user composes today in torch on the same tensors, in place on
mel energies [64, 1, 80, 201] (2 s at 100 frames/s) and [16, 1, 128, 3001] (30 s of 128 lines) with random feature lengths --
  pcen      pcen(x, Pcen(frame_rate=100), lengths, out=x)
  torch     the smoother as a conv1d with the exponential kernel b (1 - b)^k truncated at the first K with (1 - b)^K < 2^-25,
            plus the first frame's term (1 - b)^(t + 1) s[0] that makes M[0] = s[0]; then add, pow, mul, add, pow, sub and
            a where for the lengths.  The composition is approximate: the truncated tail, torch's pow, and no fixed order --
            it is compared with rtol = atol = 1e-3, not bit for bit.
_measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.  The floor of either is one read and
one write of the tensor.  Then the step
  corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=LogMel(16000, log=None), check=False)
with and without normalize=Pcen.like(features) (_measure.wall_ms, the ways in turn), and with --parent DIR (a built tree of the
parent commit) the step without normalize= by this tree's package and by the parent's, in turn:
"unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent that entry is "unmeasured".
The kernel under a profiler's counters is not measured by this tool.  One JSON document, printed and written to --out.
  python tools/bench_pcen.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/pcen.json]"""
import argparse
import math
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms


def cases(torch, pkg, dev):
    """(name, ours(), torch()) over tensors made once; both work in place on a copy of the energies refreshed by neither (a
    second pass over its own output costs the same)"""
    rng = np.random.default_rng(1)
    out = []
    how = pkg.Pcen(frame_rate=100.0)
    b, gain, bias, power, eps = (float(np.float32(a)) for a in (how.b, how.gain, how.bias, how.power, how.eps))
    K = int(math.ceil(-25.0 * math.log(2.0) / math.log(1.0 - b)))
    for shape in ((64, 1, 80, 201), (16, 1, 128, 3001)):
        B, n = shape[0], shape[-1]
        level = 2.0 ** rng.uniform(-11.0, 0.0, shape[:-1] + (1,))
        x0 = torch.from_numpy((level * rng.chisquare(2, shape)).astype(np.float32)).to(dev)
        lengths = torch.from_numpy(rng.integers(n // 2, n + 1, B)).to(dev)
        kernel = (b * (1.0 - b) ** torch.arange(K - 1, -1, -1, device=dev, dtype=torch.float32)).view(1, 1, K)
        first = ((1.0 - b) ** torch.arange(1, n + 1, device=dev, dtype=torch.float32)).view(1, n)
        t = torch.arange(n, device=dev)
        xa, xb = x0.clone(), x0.clone()

        def composition(x=xb, lengths=lengths, n=n, t=t, kernel=kernel, first=first, K=K):
            lines = x.view(-1, 1, n)
            M = torch.nn.functional.conv1d(torch.nn.functional.pad(lines, (K - 1, 0)), kernel).view(-1, n)
            M = M + first * lines[:, 0, :1]
            y = (lines.view(-1, n) * (M + eps).pow(-gain) + bias).pow(power) - bias ** power
            return x.copy_(torch.where(t.view(1, 1, 1, -1) < lengths.clamp(0, n).view(-1, 1, 1, 1), y.view(x.shape), 0.0))

        tag = "x".join(str(k) for k in shape)
        out.append((f"pcen {tag}", x0, xa, xb, lambda x=xa, lengths=lengths: pkg.pcen(x, how, lengths, out=x), composition))
    return out


def step_of(pkg, corpus, torch, pcen=False):
    spec = pkg.LogMel(16000, log=None)
    kw = dict(normalize=pkg.Pcen.like(spec)) if pcen else {}
    g = torch.Generator().manual_seed(3)
    return lambda i: corpus.random_crops(64, 32000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "pcen.json", reps=10, parent="a built tree of the parent commit: the unchanged step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    results = []
    for name, x0, xa, xb, ours, theirs in cases(torch, pkg, dev):
        a, b = ours().clone(), theirs().clone()
        close = bool(torch.allclose(a, b, rtol=1e-3, atol=1e-3))
        xa.copy_(x0)
        xb.copy_(x0)
        ms = event_ms(torch, stream, {"kernel": ours, "torch_composition": theirs}, args.steps, args.warmup, args.reps, alternate=False)
        k, c = stats(ms["kernel"]), stats(ms["torch_composition"])
        floor_bytes = 2 * 4 * x0.numel()
        results.append({"case": name, "agrees_with_torch": close, "ms_per_call_events_around_reps_calls": {"kernel": k, "torch_composition": c},
                        "kernel_median_below_torch_p10": bool(k["median"] < c["p10"]), "bytes_read_and_written_once": floor_bytes,
                        "kernel_gb_per_s_at_median": round(floor_bytes / (k["median"] * 1e-3) / 1e9, 1)})
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "torch_composition_is_approximate": "truncated exponential kernel, torch.pow, no fixed order: compared with rtol = atol = 1e-3",
           "unmeasured": ["the kernel under a profiler's counters"], "results": results}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as f:
                f.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_pcen": step_of(pkg, corpus, torch, pcen=True)}, args.steps, args.warmup)
            doc["step_wall_ms"] = {k: stats(v) for k, v in ms.items()}
            doc["unchanged_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs:
                    ms = wall_ms(torch, {"this": step_of(pkg, corpus, torch), "parent": step_of(parent, theirs, torch)}, args.steps, args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["unchanged_step_wall_ms"] = both
                    doc["unchanged_step_overlaps_parent"] = overlap(both["this"], both["parent"])
            else:
                doc["unmeasured"].append("the unchanged step against a tree of the parent commit (--parent)")
    emit(doc, args.out)


if __name__ == "__main__":
    main()
