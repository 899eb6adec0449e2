"""What noise at a target signal-to-noise ratio costs, per call and per training step --
  call      the alacgpu_mix_device call alone (ctx.mix_device, in place, the ratio given) on [64, 1, 32000] and [16, 1, 480000]
            with random lengths for the signal and the noise, against what a user writes today in torch on the same tensors:
            masks from the lengths, masked squares and sums, the gain, a gather of the noise at i mod vn and an add.
            _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=spec, check=False) with mix=AddNoise(a second
            corpus, (5, 20)) and without: _measure.wall_ms, median and p10 .. p90.  With --parent DIR (a built tree of the
            parent commit) the call without mix on the parent's package as `parent`, alternating with the others: nothing that
            existed may have moved.
One JSON document, printed and written to --out.
  python tools/bench_mix.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/mix.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, inside, load_parent, make_file, stats, wall_ms


def composition(torch, x, n, ratio, lengths, nlen, out):
    """The torch composition on x [B, C, T], n [B, Cn, T]: out = x + g n[.., i mod vn] below lengths, x behind them"""
    B, C, T = x.shape
    Cn = n.shape[1]
    i = torch.arange(T, device=x.device)
    v, vn = lengths.clamp(0, T), nlen.clamp(0, T)
    mx, mn = (i < v[:, None])[:, None, :], (i < vn[:, None])[:, None, :]
    ps = torch.where(mx, x * x, 0.0).sum((1, 2)) / (C * v).to(torch.float32)
    pn = torch.where(mn, n * n, 0.0).sum((1, 2)) / (Cn * vn).to(torch.float32)
    g = torch.where((ratio == 0) | (v == 0) | (vn == 0) | (pn == 0), 0.0, ratio * torch.sqrt(ps / pn))
    idx = (i[None, :] % vn.clamp(min=1)[:, None])[:, None, :].expand(B, C, T)
    tiled = torch.gather(n.expand(B, C, T), 2, idx)
    return torch.where(mx & (g != 0)[:, None, None], x + g[:, None, None] * tiled, x, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=30.0)
    arguments(ap, "mix.json", reps=10, parent="a built tree of the parent commit: its step without mix alternates with this tree's")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth
    from alac.net_amd.mix import snr_ratio

    synth.build()
    dev, stream = device(torch)
    rng = np.random.default_rng(1)

    # ---- the call alone --------------------------------------------------------------------------------------------------------
    calls = []
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        for B, T in ((64, 32000), (16, 480000)):
            x = torch.from_numpy(rng.uniform(-1, 1, (B, 1, T)).astype(np.float32)).to(dev)
            n = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 1, T)).astype(np.float32)).to(dev)
            lengths = torch.from_numpy(rng.integers(T // 4, T + 1, B)).to(dev)
            nlen = torch.from_numpy(rng.integers(T // 4, T + 1, B)).to(dev)
            ratio = snr_ratio(torch.from_numpy(rng.uniform(5, 20, B).astype(np.float32)), B, dev)
            res, res_t = torch.empty_like(x), torch.empty_like(x)
            ours = lambda: ctx.mix_device(x, res, n, B, 1, 1, T, T, T, lengths, nlen, ratio, stream=stream.cuda_stream)
            theirs = lambda: composition(torch, x, n, ratio, lengths, nlen, res_t)
            ours(), theirs()
            close = bool(torch.allclose(res, res_t, rtol=1e-4, atol=1e-5))
            ms = event_ms(torch, stream, {"mix_call": ours, "torch_composition": theirs}, args.steps, args.warmup, args.reps,
                          alternate=False)
            k, c = stats(ms["mix_call"]), stats(ms["torch_composition"])
            least = 4.0 * float(2 * lengths.clamp(max=T).sum() + torch.minimum(lengths, nlen).sum())      # read x and n, write y
            calls.append({"shape": [B, 1, T], "agrees_with_torch": close, "ms_per_call_events_around_reps_calls": {"mix_call": k, "torch_composition": c},
                          "mix_call_median_below_torch_median": bool(k["median"] < c["median"]),
                          "least_bytes": int(least), "mix_call_gb_per_s_of_least_bytes": round(least / k["median"] / 1e6, 1)})

    # ---- the step --------------------------------------------------------------------------------------------------------------
    rate, R, B, L = 44100, 16000, 64, 32000
    T = int(args.seconds * rate)
    distinct, distinct_noise = [make_file(synth, T, 11 + k) for k in range(2)], [make_file(synth, T // 2, 21 + k) for k in range(2)]
    blobs = [distinct[f % 2] for f in range(args.files)]
    corpus, noise = pkg.Corpus(blobs), pkg.Corpus([distinct_noise[f % 2] for f in range(max(args.files // 2, 1))])
    parent_pkg = load_parent(args.parent) if args.parent else None
    parent = parent_pkg.Corpus(blobs) if args.parent else None
    spec = pkg.LogMel(R, 400, 160, 80)
    aug = pkg.AddNoise(noise, (5, 20))
    kw = dict(sample_rate=R, mono=True, features=spec, check=False)
    ways = {"mix": lambda i: corpus.random_crops(B, L, mix=aug, **kw)[0], "without": lambda i: corpus.random_crops(B, L, **kw)[0]}
    if parent is not None:
        parent_spec = parent_pkg.LogMel(R, 400, 160, 80)
        ways["parent"] = lambda i: parent.random_crops(B, L, sample_rate=R, mono=True, features=parent_spec, check=False)[0]
    wall = wall_ms(torch, ways, args.steps, args.warmup)
    step = {"step": "random_crops(64, 32000, sample_rate=16000, mono=True, features=LogMel(16000, 400, 160, 80), check=False)",
            "wall_ms": {m: stats(v) for m, v in wall.items()}}
    if parent is not None:
        step["without_median_inside_parent_p10_p90"] = inside(step["wall_ms"]["parent"], step["wall_ms"]["without"])
    corpus.close(), noise.close()
    if parent is not None:
        parent.close()
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "calls": calls, "step": step}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
