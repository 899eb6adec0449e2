"""What Kaldi's pitch features cost --
  call      kaldi_pitch(x, KaldiPitch(16000), lengths, out=track) on [64, 1, 32000] with random lengths in 16000 .. 32000 and
            its stages apart: kaldi_pitch_nccf (the downsampler and the NCCF, two launches), kaldi_pitch_decode on those NCCFs,
            kaldi_pitch_process on that raw track.  _measure.event_ms, one way after the other: median and p10 .. p90 of the
            time per call.  "decode_us_per_frame" is the decode's median over its frames: a chain of frames, as pYIN's decode is
            (15 us a frame in profiles/pyin.json).
  torch     the same pipeline composed in torch on 2 rows: conv1d with the downsampler's taps, unfold, the sums of the NCCF,
            the interpolation as a matmul, and a Python loop over the frames for the recursion (the walk back left out);
            "torch_scaled_to_64_rows" is that time times 32 -- a scaling, not a measurement.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=KaldiFbank(16000), check=False) without f0=,
            with f0=Yin.like(spec) and with f0=KaldiPitch.like(spec) (_measure.wall_ms, the ways in turn), and with --parent DIR
            (a built tree of the parent commit) the step with f0=Yin.like(spec) by this tree's package and by the parent's, in
            turn.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_kaldi_pitch.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/kaldi_pitch.json]"""
import argparse
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms


def step_of(pkg, corpus, torch, f0=None):
    spec = pkg.KaldiFbank(16000)
    g = torch.Generator().manual_seed(3)
    kw = {} if f0 is None else {"f0": getattr(pkg, f0).like(spec)}
    return lambda i: corpus.random_crops(64, 32000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "kaldi_pitch.json", reps=10, parent="a built tree of the parent commit: the step with f0=Yin is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    B, T, rate = 64, 32000, 16000
    spec = pkg.KaldiPitch(rate)
    t = np.arange(T) / rate
    f = rng.uniform(80.0, 300.0, (B, 1, 1))
    x = torch.from_numpy((0.4 * np.sin(2 * np.pi * f * t) + 0.05 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    lengths = torch.from_numpy(rng.integers(T // 2, T + 1, B)).to(dev)
    F, S = int(spec.frames(T)), spec.n_states
    track = torch.empty((B, 1, spec.lines, F), dtype=torch.float32, device=dev)
    counts = spec.lengths(lengths)
    nccf = pkg.kaldi_pitch_nccf(x, spec, lengths)
    raw = pkg.kaldi_pitch_decode(nccf, spec, counts)
    tab = spec.tables()
    down = torch.from_numpy(tab["down"][0]).to(dev)[None, None]
    first = int(tab["down_first"][0])
    W, L0, L1 = spec.window, spec.first_lag, spec.last_lag
    up = torch.zeros((spec.n_lags, S), device=dev)
    for k in range(tab["up"].shape[1]):
        up[torch.from_numpy(tab["up_first"] + k).to(dev), torch.arange(S, device=dev)] = torch.from_numpy(tab["up"][:, k]).to(dev)
    sl = torch.from_numpy(tab["sl"]).to(dev)
    at = torch.arange(S, device=dev)
    cost = ((at[:, None] - at[None, :]) ** 2).float() * float(tab["head"][0])

    def composed():
        y = x[:2]
        d = torch.nn.functional.conv1d(torch.nn.functional.pad(y, (-first, 0)), down, stride=4)[:, 0]
        ballast = ((d * d).mean(-1) - d.mean(-1) ** 2) * W
        ballast = (ballast * ballast * 7000.0)[:, None, None]
        fr = d.unfold(-1, spec.span, spec.shift)
        z = fr - fr[..., :W].mean(-1, keepdim=True)
        lagged = z.unfold(-1, W, 1)[..., L0:L1 + 1, :]
        inner = (lagged * z[..., None, :W]).sum(-1)
        norm = (z[..., :W] ** 2).sum(-1, keepdim=True) * (lagged ** 2).sum(-1)
        n = (inner / torch.sqrt(norm + ballast)) @ up
        local = 1.0 - n + sl * n
        fwd = local[:, 0]
        for k in range(1, local.shape[1]):
            fwd = (fwd[:, None, :] + cost).min(-1)[0] + local[:, k]
            fwd = fwd - fwd.min(-1, keepdim=True)[0]
        return fwd.argmin(-1)

    ways = {"kaldi_pitch": lambda: pkg.kaldi_pitch(x, spec, lengths, out=track), "nccf": lambda: pkg.kaldi_pitch_nccf(x, spec, lengths),
            "decode": lambda: pkg.kaldi_pitch_decode(nccf, spec, counts), "process": lambda: pkg.kaldi_pitch_process(raw, spec, counts)}
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False)
    calls = {k: stats(v) for k, v in ms.items()}
    ms = event_ms(torch, stream, {"torch_pipeline_2_rows": composed}, max(args.steps // 20, 3), 2, 1, alternate=False)
    calls["torch_pipeline_2_rows"] = stats(ms["torch_pipeline_2_rows"])
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "spec": repr(spec), "frames": F, "n_states": S, "ms_per_call_events_around_reps_calls": calls,
           "decode_us_per_frame": round(1000.0 * calls["decode"]["median"] / F, 2),
           "torch_scaled_to_64_rows": round(32 * calls["torch_pipeline_2_rows"]["median"], 1),
           "unmeasured": ["the three kernels under a profiler's counters", "the walk back apart from the recursion",
                          "rates other than 16 kHz"]}
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as fh:
                fh.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_yin": step_of(pkg, corpus, torch, "Yin"),
                                 "step_kaldi_pitch": step_of(pkg, corpus, torch, "KaldiPitch")}, args.steps, args.warmup)
            both = {k: stats(v) for k, v in ms.items()}
            doc["step_wall_ms"] = both
            doc["step_kaldi_pitch_multiple_of_step"] = round(both["step_kaldi_pitch"]["median"] / both["step"]["median"], 3)
            doc["yin_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs:
                    ms = wall_ms(torch, {"this": step_of(pkg, corpus, torch, "Yin"), "parent": step_of(parent, theirs, torch, "Yin")},
                                 args.steps, args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["yin_step_wall_ms"] = both
                    doc["yin_step_overlaps_parent"] = overlap(both["this"], both["parent"])
    emit(doc, args.out)


if __name__ == "__main__":
    main()
