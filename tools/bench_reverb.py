"""What room reverberation costs, per call and per training step --
  call      the alacgpu_reverb_device call alone (ctx.reverb_device, in place) on [64, 1, 32000] with responses of K = 8000 and
            K = 16000 frames and random lengths for both, against what a user writes today in torch on the same tensors:
            torch.fft.rfft of both at a common length, their product, irfft, the shift to the largest tap by a gather, the
            energy gain and a `where` over the lengths.  _measure.event_ms, the two ways alternating inside every repetition:
            median and p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=spec, check=False) with
            reverb=Reverb(a corpus of responses, max_seconds=0.5), without,
            and with all four stages (reverb=, mix=AddNoise(the corpus itself, (5, 20)), normalize=MeanVar()):
            _measure.wall_ms, median and p10 .. p90.  With --parent DIR (a built tree of the parent commit) the same three
            steps on the parent's package as `parent_...`, alternating with the others: nothing that existed may have moved.
One JSON document, printed and written to --out.
  python tools/bench_reverb.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/reverb.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, not_above, stats, wall_ms


def composition(torch, x, h, lengths, hlen, out):
    """The torch composition on x [B, C, T], h [B, Ch, K]: out = g (h * x)[i + d] below lengths, x behind them"""
    B, C, T = x.shape
    K = h.shape[2]
    i, k = torch.arange(T, device=x.device), torch.arange(K, device=x.device)
    v, vh = lengths.clamp(0, T), hlen.clamp(0, K)
    mx, mh = (i < v[:, None])[:, None, :], (k < vh[:, None])[:, None, :]
    xs, hs = torch.where(mx, x, 0.0), torch.where(mh, h, 0.0)
    n = T + K - 1
    w = torch.fft.irfft(torch.fft.rfft(xs, n) * torch.fft.rfft(hs, n), n)
    d = hs[:, 0].abs().argmax(1)
    e = (hs * hs).sum((1, 2)) / h.shape[1]
    g = torch.rsqrt(e)
    idx = (i[None, :] + d[:, None])[:, None, :].expand(B, C, T)
    y = g[:, None, None] * torch.gather(w, 2, idx)
    live = (v > 0) & (vh > 0) & (e > 0) & torch.isfinite(e)
    return torch.where(mx & live[:, None, None], y, x, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=30.0)
    arguments(ap, "reverb.json", reps=10, parent="a built tree of the parent commit: its step without reverb alternates with this tree's")
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
        B, T = 64, 32000
        for K in (8000, 16000):
            x0 = torch.from_numpy(rng.uniform(-1, 1, (B, 1, T)).astype(np.float32)).to(dev)
            taps = rng.standard_normal((B, 1, K)) * np.exp(-np.arange(K) / (K / 6.0))
            taps[:, 0, 40] = 4.0
            h = torch.from_numpy(taps.astype(np.float32)).to(dev)
            lengths = torch.from_numpy(rng.integers(T // 4, T + 1, B)).to(dev)
            hlen = torch.from_numpy(rng.integers(K // 2, K + 1, B)).to(dev)
            res, res_t = torch.empty_like(x0), torch.empty_like(x0)
            ctx.reverb_device(x0, res, h, B, 1, 1, T, K, T, K, lengths, hlen, stream=stream.cuda_stream)
            composition(torch, x0, h, lengths, hlen, res_t)
            close = bool(torch.allclose(res, res_t, rtol=1e-3, atol=1e-4))
            x = x0.clone()                                 # in place, as crops() calls it: the values drift, the work does not
            ours = lambda: ctx.reverb_device(x, x, h, B, 1, 1, T, K, T, K, lengths, hlen, stream=stream.cuda_stream)
            theirs = lambda: composition(torch, x0, h, lengths, hlen, res_t)
            ms = event_ms(torch, stream, {"reverb_call": ours, "torch_composition": theirs}, args.steps, args.warmup, args.reps,
                          alternate=True, before={"reverb_call": lambda: x.copy_(x0)})
            r, c = stats(ms["reverb_call"]), stats(ms["torch_composition"])
            calls.append({"shape": [B, 1, T], "rir_frames": K, "agrees_with_torch": close,
                          "ms_per_call_events_around_reps_calls": {"reverb_call": r, "torch_composition": c},
                          "reverb_call_median_below_torch_p10": bool(r["median"] < c["p10"])})

    # ---- the step --------------------------------------------------------------------------------------------------------------
    rate, R, B, L = 44100, 16000, 64, 32000
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    blobs = [distinct[f % 2] for f in range(args.files)]
    rir_files = [make_file(synth, 2 * R, 31 + k) for k in range(4)]
    corpus, rirs = pkg.Corpus(blobs), pkg.Corpus(rir_files)
    kw = dict(sample_rate=R, mono=True, check=False)

    def steps(p, corpus, rirs):
        """The three steps on the package p: with reverb=, without, and with all four stages (the noise from the corpus itself)"""
        spec, aug = p.LogMel(R, 400, 160, 80), p.Reverb(rirs, max_seconds=0.5)
        add, how = p.AddNoise(corpus, (5, 20)), p.MeanVar()
        return {"reverb": lambda i: corpus.random_crops(B, L, reverb=aug, features=spec, **kw)[0],
                "without": lambda i: corpus.random_crops(B, L, features=spec, **kw)[0],
                "all_stages": lambda i: corpus.random_crops(B, L, reverb=aug, mix=add, features=spec, normalize=how, **kw)[0]}

    ways = steps(pkg, corpus, rirs)
    parent = parent_rirs = None
    if args.parent:
        parent_pkg = load_parent(args.parent)
        parent, parent_rirs = parent_pkg.Corpus(blobs), parent_pkg.Corpus(rir_files)
        ways.update({"parent_" + m: fn for m, fn in steps(parent_pkg, parent, parent_rirs).items()})
    wall = wall_ms(torch, ways, args.steps, args.warmup)
    step = {"step": "random_crops(64, 32000, sample_rate=16000, mono=True, features=LogMel(16000, 400, 160, 80), check=False)",
            "reverb": "Reverb(4 stereo files of 32000 frames at 44.1 kHz, max_seconds=0.5): K = 8000, taken as one channel",
            "all_stages": "reverb= as above, mix=AddNoise(the corpus itself, (5, 20)), normalize=MeanVar()",
            "wall_ms": {m: stats(v) for m, v in wall.items()}}
    if parent is not None:
        for m in ("reverb", "without", "all_stages"):
            step[m + "_median_inside_parent_p10_p90_or_below"] = not_above(step["wall_ms"]["parent_" + m], step["wall_ms"][m])
    corpus.close(), rirs.close()
    if parent is not None:
        parent.close(), parent_rirs.close()
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "calls": calls, "step": step}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
