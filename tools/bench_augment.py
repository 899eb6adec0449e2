"""What SpecAugment costs, per call and per training step --
  call      the alacgpu_specaugment_device call alone (ctx.specaugment_device, in place, the draws given) on [64, 1, 80, 201] and
            on [16, 1, 128, 3000], the slice [..., :3000] of 3001, with random lengths; masks only (two of each kind) and with
            time_warp=5 as well, against what a user writes today in torch on the same tensors: broadcast compares and a `where`
            for the masks (a masked fill), a batched index computation, two gathers and a lerp for the warp (float32 positions: close to the
            kernel's, not its bits).  _measure.event_ms, one way after the other: median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=spec, normalize=MeanVar(), check=False) with
            augment=SpecAugment(time_warp=5) and without: _measure.wall_ms, median and p10 .. p90.  With --parent DIR (a built tree of the parent commit)
            the call without augment on the parent's package as `parent`, alternating with the others: nothing that existed may
            have moved.  Without --parent the document says that it was not measured.
One JSON document, printed and written to --out.
  python tools/bench_augment.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/augment.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, inside, load_parent, make_file, stats, wall_ms


def composition(torch, x, warp, freq, time_, lengths, fill, with_warp):
    """The torch composition on x [B, C, M, N], in place as far as torch goes: the warp out of place (a gather needs its
    source whole), the masks as one masked fill over the tensor"""
    B, C, M, N = x.shape
    tau = lengths.clamp(0, N)
    t = torch.arange(N, device=x.device)
    if with_warp:
        c, c1 = warp[:, 0:1].to(torch.float32), warp[:, 1:2].to(torch.float32)
        last = (tau[:, None] - 1).to(torch.float32)
        tf = t[None, :].to(torch.float32)
        s = torch.where(tf <= c1, tf * c / c1.clamp(min=1), c + (tf - c1) * (last - c) / (last - c1).clamp(min=1))
        s = torch.where((warp[:, 0:1] > 0) & (t[None, :] < tau[:, None]), s, tf)
        i = s.floor().clamp(0, N - 1).to(torch.int64)
        f = (s - i)[:, None, None, :]
        i0 = i[:, None, None, :].expand(B, C, M, N)
        i1 = (i + 1).clamp(max=N - 1)[:, None, None, :].expand(B, C, M, N)
        x.copy_(torch.lerp(torch.gather(x, 3, i0), torch.gather(x, 3, i1), f))
    m = torch.arange(M, device=x.device)
    fm = ((m[None, None, :] >= freq[:, :, 0:1]) & (m[None, None, :] < (freq[:, :, 0:1] + freq[:, :, 1:2]))).any(1)       # [B, M]
    tm = ((t[None, None, :] >= time_[:, :, 0:1]) & (t[None, None, :] < (time_[:, :, 0:1] + time_[:, :, 1:2]))).any(1)   # [B, N]
    mask = (fm[:, :, None] | tm[:, None, :]) & (t[None, None, :] < tau[:, None, None])
    return x.masked_fill_(mask[:, None], fill)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=30.0)
    arguments(ap, "augment.json", reps=10, parent="a built tree of the parent commit: its step without augment alternates with this tree's")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    dev, stream = device(torch)
    rng = np.random.default_rng(1)

    # ---- the call alone --------------------------------------------------------------------------------------------------------
    calls = []
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        for (B, M, N), sliced in (((64, 80, 201), False), ((16, 128, 3000), True)):
            S = N + 1 if sliced else N
            base = torch.from_numpy(rng.standard_normal((B, 1, M, S)).astype(np.float32)).to(dev)
            x = base[..., :N]
            lengths = torch.from_numpy(rng.integers(N // 4, N + 1, B)).to(dev)
            for W in (0, 5):
                spec = pkg.SpecAugment(time_warp=W)
                warp, freq, time_ = spec.draw(M, lengths, generator=torch.Generator(device=dev).manual_seed(2))
                d_warp = warp if W else None
                theirs_x = x.clone()
                ours_x = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=dev).copy_(x)      # (x's layout: the slice)
                ours = lambda: ctx.specaugment_device(ours_x, ours_x, B, 1, M, S, N, lengths, d_warp, freq, time_, 0.0, stream=stream.cuda_stream)
                theirs = lambda: composition(torch, theirs_x, warp, freq, time_, lengths, 0.0, bool(W))
                ours(), theirs()
                close = bool(torch.allclose(ours_x, theirs_x, rtol=1e-3, atol=1e-3))
                ms = event_ms(torch, stream, {"specaugment_call": ours, "torch_composition": theirs}, args.steps, args.warmup, args.reps,
                              alternate=False)
                k, c = stats(ms["specaugment_call"]), stats(ms["torch_composition"])
                calls.append({"shape": [B, 1, M, N], "line_stride": S, "time_warp": W, "in_place": True,
                              "first_call_agrees_with_torch_to_1e-3": close,
                              "ms_per_call_events_around_reps_calls": {"specaugment_call": k, "torch_composition": c},
                              "specaugment_call_median_below_torch_median": bool(k["median"] < c["median"])})

    # ---- the step --------------------------------------------------------------------------------------------------------------
    rate, R, B, L = 44100, 16000, 64, 32000
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    blobs = [distinct[f % 2] for f in range(args.files)]
    corpus = pkg.Corpus(blobs)
    parent_pkg = load_parent(args.parent) if args.parent else None
    parent = parent_pkg.Corpus(blobs) if args.parent else None
    spec = pkg.LogMel(R, 400, 160, 80)
    aug = pkg.SpecAugment(time_warp=5)
    kw = dict(sample_rate=R, mono=True, features=spec, normalize=pkg.MeanVar(), check=False)
    ways = {"augment": lambda i: corpus.random_crops(B, L, augment=aug, **kw)[0], "without": lambda i: corpus.random_crops(B, L, **kw)[0]}
    if parent is not None:
        parent_kw = dict(sample_rate=R, mono=True, features=parent_pkg.LogMel(R, 400, 160, 80), normalize=parent_pkg.MeanVar(), check=False)
        ways["parent"] = lambda i: parent.random_crops(B, L, **parent_kw)[0]
    wall = wall_ms(torch, ways, args.steps, args.warmup)
    step = {"step": "random_crops(64, 32000, sample_rate=16000, mono=True, features=LogMel(16000, 400, 160, 80), normalize=MeanVar(), check=False)",
            "augment": "SpecAugment(time_warp=5)", "wall_ms": {m: stats(v) for m, v in wall.items()}}
    if parent is not None:
        step["without_median_inside_parent_p10_p90"] = inside(step["wall_ms"]["parent"], step["wall_ms"]["without"])
    else:
        step["parent"] = "not measured: no tree of the parent commit was given (--parent)"
    corpus.close()
    if parent is not None:
        parent.close()
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "calls": calls, "step": step}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
