"""What the sliding-window CMVN, the energy VAD and the selection of the voiced frames cost next to what a user writes today in
torch on the same tensors, on features [64, 1, 30, 298] (3 s of MFCCs, the x-vector recipes' shape) and [64, 1, 80, 2998]
(30 s of 80 lines) with random feature lengths --
  sliding   normalize(x, SlidingMeanVar.xvector(), lengths)   against a cumsum over the frames, an index computation for every
            frame's window and the difference of two gathers (float32 prefix sums: what sliding.py's bound rules out)
  vad       vad_energy(x, EnergyVad.voxceleb(), lengths)      against a masked mean, a compare, unfold over the padded decisions
            and a second compare
  select    select_frames(x, mask, lengths)                   against a stable sort of the frames by "not voiced" and a gather
            (the compaction without a host sync; a boolean masked_scatter needs the row counts on the host)
each into preallocated results where torch allows it.  _measure.event_ms, one way after the other: median and p10 .. p90 of
the time per call.  Then the README's step,
  corpus.random_crops(64, 48000, sample_rate=16000, mono=True, features=KaldiMfcc(16000, n_mels=30, n_ceps=30), check=False)
with and without vad=EnergyVad.voxceleb(), normalize=SlidingMeanVar.xvector() (_measure.wall_ms, the ways in turn), and with
--parent DIR (a built tree of the parent commit) the step without either by this tree's package and by the parent's, in turn:
"unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent that entry is "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_sliding_vad.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/sliding_vad.json]"""
import argparse
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms


def cases(torch, pkg, dev):
    """(name, ours(), torch()) over tensors made once"""
    rng = np.random.default_rng(1)
    out = []
    for shape in ((64, 1, 30, 298), (64, 1, 80, 2998)):
        B, n = shape[0], shape[-1]
        x = torch.from_numpy((8.0 + 6.0 * rng.uniform(-1, 1, shape)).astype(np.float32)).to(dev)
        lengths = torch.from_numpy(rng.integers(n // 2, n + 1, B)).to(dev)
        how, vad = pkg.SlidingMeanVar.xvector(), pkg.EnergyVad.voxceleb()
        res = torch.empty_like(x)
        mask = pkg.vad_energy(x, vad, lengths)
        t = torch.arange(n, device=dev)

        def sliding_torch(x=x, lengths=lengths, n=n, t=t, W=how.window):
            v = lengths.clamp(0, n).view(-1, 1)
            s = (t - W // 2).view(1, -1).expand(v.shape[0], n)
            e = s + W
            e = torch.where(s < 0, e - s, e)
            s = s.clamp(min=0)
            over = e > v
            s = torch.where(over, s - (e - v), s).clamp(min=0)
            e = torch.where(over, v, e)
            c = torch.nn.functional.pad(x.cumsum(-1), (1, 0))
            idx = lambda k: k.view(v.shape[0], 1, 1, n).expand(x.shape)
            m = (c.gather(-1, idx(e)) - c.gather(-1, idx(s))) / idx(e - s).to(torch.float32)
            return torch.where(t.view(1, 1, 1, -1) < v.view(-1, 1, 1, 1), x - m, 0.0)

        def vad_torch(x=x, lengths=lengths, n=n, t=t, vad=vad):
            v = lengths.clamp(0, n).view(-1, 1)
            E = x[:, 0, vad.line, :]
            live = t.view(1, -1) < v
            thr = vad.energy_threshold + vad.energy_mean_scale * torch.where(live, E, 0.0).sum(-1, keepdim=True) / v.to(torch.float32)
            c = vad.frames_context
            pad = lambda a: torch.nn.functional.pad(a.to(torch.float32), (c, c)).unfold(-1, 2 * c + 1, 1).sum(-1)
            num, den = pad((E > thr) & live), pad(live)
            return ((num >= den * vad.proportion_threshold) & live).to(torch.uint8)

        def select_torch(x=x, mask=mask, lengths=lengths, n=n, t=t):
            keep = (mask != 0) & (t.view(1, -1) < lengths.clamp(0, n).view(-1, 1))
            order = torch.sort((~keep).to(torch.uint8), dim=-1, stable=True).indices
            count = keep.sum(-1)
            y = x.gather(-1, order.view(x.shape[0], 1, 1, n).expand(x.shape))
            return torch.where(t.view(1, 1, 1, -1) < count.view(-1, 1, 1, 1), y, 0.0), count

        tag = "x".join(str(k) for k in shape)
        out.append((f"sliding {tag}", lambda x=x, how=how, lengths=lengths, res=res: pkg.normalize(x, how, lengths, out=res), sliding_torch))
        out.append((f"vad {tag}", lambda x=x, vad=vad, lengths=lengths: pkg.vad_energy(x, vad, lengths), vad_torch))
        out.append((f"select {tag}", lambda x=x, mask=mask, lengths=lengths, res=res: pkg.select_frames(x, mask, lengths, out=res)[0],
                    lambda f=select_torch: f()[0]))
    return out


def step_of(pkg, corpus, torch, **kw):
    spec = pkg.KaldiMfcc(16000, n_mels=30, n_ceps=30)
    g = torch.Generator().manual_seed(3)
    return lambda i: corpus.random_crops(64, 48000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "sliding_vad.json", reps=10, parent="a built tree of the parent commit: the unchanged step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    results = []
    for name, ours, theirs in cases(torch, pkg, dev):
        a, b = ours().clone(), theirs().clone()
        close = bool(torch.allclose(a.float(), b.float(), rtol=1e-3, atol=1e-3, equal_nan=True))
        ms = event_ms(torch, stream, {"kernel": ours, "torch_composition": theirs}, args.steps, args.warmup, args.reps, alternate=False)
        k, c = stats(ms["kernel"]), stats(ms["torch_composition"])
        results.append({"case": name, "agrees_with_torch": close, "ms_per_call_events_around_reps_calls": {"kernel": k, "torch_composition": c},
                        "kernel_median_below_torch_p10": bool(k["median"] < c["p10"])})
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "results": results}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as f:
                f.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ways = {"step": step_of(pkg, corpus, torch),
                    "step_vad_sliding": step_of(pkg, corpus, torch, vad=pkg.EnergyVad.voxceleb(), normalize=pkg.SlidingMeanVar.xvector())}
            ms = wall_ms(torch, ways, args.steps, args.warmup)
            doc["readme_step_wall_ms"] = {k: stats(v) for k, v in ms.items()}
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
