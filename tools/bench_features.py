"""What log-mel features of crops cost per training step: B random crops at 16 kHz mono out of synthetic M4A files (stereo
16-bit at 44.1 kHz, 4096-frame packets, 60 s each), device index tensors and check=False throughout, LogMel(16000, 400, 160,
80), per shape (B crops of a duration) --
  features     corpus.crops(..., sample_rate=16000, mono=True, features=spec): the new step
  crops        corpus.crops(..., sample_rate=16000, mono=True): the step without the features, on the same build.  With
               --parent DIR (a built tree of the parent commit) the same call on the parent's package as `parent`, alternating
               with this one: nothing that existed may have moved
  torch        for comparison, what a user writes today on the same crops: torch.stft(center, reflect, periodic Hann) ->
               abs()^2 -> matmul with spec.fb -> clamp(min=floor) -> log
Wall time of a step: _measure.wall_ms, median and p10 .. p90.  Then, over one step's crops, _measure.event_ms, one way after
the other: the alacgpu_logmel_device call alone, and the torch composition alone.  One JSON document, printed and written to
--out.
  python tools/bench_features.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/corpus_features.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, inside, load_parent, make_file, stats, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--shape", action="append", help="BxSECONDS, repeatable (default 64x2 and 256x1)")
    arguments(ap, "corpus_features.json", reps=10, parent="a built tree of the parent commit: its crops alternate with this tree's")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    dev, stream = device(torch)
    rate, R = 44100, 16000
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    blobs = [distinct[f % 2] for f in range(args.files)]
    corpus = pkg.Corpus(blobs)
    parent = load_parent(args.parent).Corpus(blobs) if args.parent else None
    spec = pkg.LogMel(R, 400, 160, 80)
    window, basis, fb = spec.device_tables(dev)
    hann = torch.hann_window(spec.n_fft, periodic=True, device=dev)

    def compose(x):
        """x [B, 1, L] -> [B, 1, n_mels, T']"""
        s = torch.stft(x[:, 0], spec.n_fft, spec.hop_length, window=hann, center=True, pad_mode="reflect", return_complex=True)
        return torch.matmul(fb, s.abs() ** 2).clamp(min=spec.floor).log()[:, None]

    results = []
    for B, seconds in [tuple(int(x) for x in s.split("x")) for s in (args.shape or ["64x2", "256x1"])]:
        n_steps = args.steps + args.warmup
        rng = np.random.default_rng(B + seconds)
        L = seconds * R
        files = [torch.from_numpy(rng.integers(0, args.files, B)).to(dev) for _ in range(n_steps)]
        offs = [torch.from_numpy((rng.random(B) * (-(-R * T // rate) - L + 1)).astype(np.int64)).to(dev) for _ in range(n_steps)]
        kw = dict(check=False, sample_rate=R, mono=True)
        ways = {"features": lambda i: corpus.crops(files[i], offs[i], L, features=spec, **kw)[0],
                "crops": lambda i: corpus.crops(files[i], offs[i], L, **kw)[0]}
        if parent is not None:
            ways["parent"] = lambda i: parent.crops(files[i], offs[i], L, **kw)[0]
            assert torch.equal(ways["crops"](0), ways["parent"](0)), "the crops differ from the parent's"
        ways["torch"] = lambda i: compose(corpus.crops(files[i], offs[i], L, **kw)[0])
        ours, theirs = ways["features"](0), ways["torch"](0)
        worst = float((ours - theirs).abs().max())
        wall = wall_ms(torch, ways, args.steps, args.warmup)
        r = {"crops": B, "seconds": seconds, "feature_frames": spec.frames(L), "max_abs_difference_to_torch_in_ln": round(worst, 6),
             "wall_ms": {m: stats(v) for m, v in wall.items()}}
        if parent is not None:
            r["crops_median_inside_parent_p10_p90"] = inside(r["wall_ms"]["parent"], r["wall_ms"]["crops"])
        # the two feature computations alone, over one step's crops
        pcm = corpus.crops(files[0], offs[0], L, **kw)[0]
        out = torch.empty((B, 1, spec.n_mels, spec.frames(L)), dtype=torch.float32, device=dev)

        def native():
            corpus._gpu.logmel_device(pcm, B, 1, L, L, spec.n_fft, spec.hop_length, spec.n_mels, window, basis, fb, spec.log_mode,
                                      spec.floor, out, spec.frames(L), stream=stream.cuda_stream)

        ms = event_ms(torch, stream, {"logmel_call": native, "torch_composition": lambda: compose(pcm)}, args.steps, args.warmup, args.reps,
                      alternate=False)
        k, c = stats(ms["logmel_call"]), stats(ms["torch_composition"])
        flop = 2.0 * B * spec.frames(L) * (spec.n_fft * 2 * spec.n_bins + spec.n_mels * spec.n_bins)
        r["alone_ms_events_around_reps_calls"] = {"logmel_call": k, "torch_composition": c}
        r["logmel_call_tflops"] = round(flop / k["median"] / 1e9, 2)
        r["logmel_median_below_torch_p10"] = bool(k["median"] < c["p10"])
        results.append(r)
    doc = {"command": command(__file__), "files": args.files, "seconds": args.seconds,
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "spec": repr(spec), "results": results}
    corpus.close()
    if parent is not None:
        parent.close()
    emit(doc, args.out)


if __name__ == "__main__":
    main()
