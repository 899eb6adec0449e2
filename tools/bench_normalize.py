"""What the two normalisations cost next to what a user writes today in torch on the same tensors, per case --
  whisper feats 64     features [64, 1, 80, 201] (2 s at 16 kHz), normalize(x, TopDb.whisper())
  whisper slice 16     features [16, 1, 128, 3001] through the slice [..., :3000] (30 s: Whisper drops the last frame)
  cmvn feats 64        features [64, 1, 80, 201] with random feature lengths, normalize(x, MeanVar(), lengths)
  waveform 64          waveform [64, 1, 32000] with random lengths, normalize(x, MeanVar(), lengths)
against
  TopDb                amax over the row -> maximum -> mul -> add (four launches and a temporary)
  MeanVar              a mask from lengths, masked mean, masked var, where (a dozen launches)
each into a preallocated result.  _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
One JSON document, printed and written to --out.
  python tools/bench_normalize.py [--steps 200] [--warmup 20] [--out profiles/normalize.json]
Kernel times come from a run of their own under the profiler, which this tool only feeds and reads:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o normalize -- python tools/bench_normalize.py --loop 50
  python tools/bench_normalize.py --kernel-stats DIR/.../normalize_kernel_stats.csv      (adds them to --out)"""
import argparse
import csv
import json

import numpy as np

from _measure import arguments, command, device, emit, event_ms, stats


def cases(torch, pkg, dev):
    """(name, ours(), torch()) over tensors made once; both write a preallocated result"""
    rng = np.random.default_rng(1)
    out = []

    def top(name, x):
        how = pkg.TopDb.whisper()
        res, res_t = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=dev), torch.empty_like(x)

        def theirs():
            mx = x.amax(dim=tuple(range(1, x.dim())), keepdim=True)
            torch.maximum(x, mx - 8.0, out=res_t)
            return res_t.mul_(0.25).add_(1.0)

        out.append((name, lambda: pkg.normalize(x, how, out=res), theirs))

    def meanvar(name, x, lengths):
        how = pkg.MeanVar()
        n = x.shape[-1]
        res = torch.empty_like(x)
        shape = (-1,) + (1,) * (x.dim() - 1)

        def theirs():
            v = lengths.clamp(0, n).view(shape)
            mask = torch.arange(n, device=dev).view((1,) * (x.dim() - 1) + (n,)) < v
            cnt = v.to(torch.float32)
            mean = torch.where(mask, x, 0.0).sum(-1, keepdim=True) / cnt
            d = torch.where(mask, x - mean, 0.0)
            var = (d * d).sum(-1, keepdim=True) / cnt
            return d / var.sqrt()

        out.append((name, lambda: pkg.normalize(x, how, lengths, out=res), theirs))

    feats = torch.from_numpy(rng.uniform(-10, 2, (64, 1, 80, 201)).astype(np.float32)).to(dev)
    long = torch.from_numpy(rng.uniform(-10, 2, (16, 1, 128, 3001)).astype(np.float32)).to(dev)
    wave = torch.from_numpy(rng.uniform(-1, 1, (64, 1, 32000)).astype(np.float32)).to(dev)
    top("whisper feats 64", feats)
    top("whisper slice 16", long[..., :3000])
    meanvar("cmvn feats 64", feats, torch.from_numpy(rng.integers(20, 202, 64)).to(dev))
    meanvar("waveform 64", wave, torch.from_numpy(rng.integers(8000, 32001, 64)).to(dev))
    return out


def read_kernel_stats(path):
    """rocprofv3's kernel stats: name -> calls and average microseconds"""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, help="only call every case's two ways that many times (the run under the profiler)")
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel stats CSV of a --loop run: added to --out as kernel_stats")
    arguments(ap, "normalize.json", reps=10)
    args = ap.parse_args()
    if args.kernel_stats is not None:
        doc = json.load(open(args.out))
        doc["kernel_stats"] = read_kernel_stats(args.kernel_stats)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        return
    import torch

    import alac.net_amd as pkg

    dev, stream = device(torch)
    todo = cases(torch, pkg, dev)
    if args.loop:
        for name, ours, theirs in todo:
            for _ in range(args.loop):
                ours()
                theirs()
        torch.cuda.synchronize()
        return
    results = []
    for name, ours, theirs in todo:
        a, b = ours().clone(), theirs().clone()
        close = bool(torch.allclose(a, b, rtol=1e-4, atol=1e-4, equal_nan=True))
        ms = event_ms(torch, stream, {"normalize": ours, "torch_composition": theirs}, args.steps, args.warmup, args.reps, alternate=False)
        k, c = stats(ms["normalize"]), stats(ms["torch_composition"])
        results.append({"case": name, "agrees_with_torch": close, "ms_per_call_events_around_reps_calls": {"normalize": k, "torch_composition": c},
                        "normalize_median_below_torch_p10": bool(k["median"] < c["p10"])})
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "results": results}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
