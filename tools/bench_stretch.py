"""What the pitch shift and the time stretch cost --
  call      pitch_shift(x, ratios, 16000, lengths, out=x) in place on [64, 1, 32000] with random lengths in 16000 .. 32000 and
            ratios drawn from the default PitchShift, against the same thing composed in torch, written here: per distinct
            ratio torch.stft of its rows, the phase vocoder in torch operations (torchaudio's, angles and cumsum), torch.istft,
            then alac.speed_perturb and a masked copy; and time_stretch(x, ratios, lengths) alone.  x is restored from a copy in
            front of every repetition, outside the events.  _measure.event_ms, one way after the other: median and p10 .. p90
            of the time per call.  A torch composition that this build of torch cannot run is recorded as such.
  step      corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=KaldiFbank(16000), check=False) with and
            without pitch=PitchShift() (_measure.wall_ms, the ways in turn), and with --parent DIR (a built tree of the parent
            commit) the step without pitch= by this tree's package and by the parent's, in turn:
            "unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_stretch.py [--steps 200] [--warmup 20] [--parent DIR] [--out profiles/stretch.json]"""
import argparse
import math
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms


def step_of(pkg, corpus, torch, **kw):
    spec = pkg.KaldiFbank(16000)
    g = torch.Generator().manual_seed(3)
    return lambda i: corpus.random_crops(64, 32000, generator=g, sample_rate=16000, mono=True, features=spec, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def torch_vocoder(torch, X, rate, hop):
    """torchaudio.functional.phase_vocoder in torch operations: X complex [rows, K, T], rate = 1 / factor"""
    K = X.shape[1]
    steps = torch.arange(0, X.shape[2], rate, device=X.device, dtype=torch.float64)
    alphas = (steps % 1.0).to(torch.float32)
    advance = torch.linspace(0, math.pi * hop, K, device=X.device)[None, :, None]
    phase_0 = X[..., :1].angle()
    X = torch.nn.functional.pad(X, [0, 2])
    i = steps.long()
    a, b = X.index_select(2, i), X.index_select(2, i + 1)
    phase = b.angle() - a.angle() - advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi)) + advance
    acc = torch.cumsum(torch.cat([phase_0, phase[..., :-1]], dim=-1), -1)
    return torch.polar(alphas * b.abs() + (1 - alphas) * a.abs(), acc)


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "stretch.json", reps=4, parent="a built tree of the parent commit: the unchanged step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    B, T, rate, n_fft = 64, 32000, 16000, 512
    hop = n_fft // 4
    x = torch.from_numpy((0.1 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    host_lengths = rng.integers(T // 2, T + 1, B)
    lengths = torch.from_numpy(host_lengths).to(dev)
    x0 = x.clone()
    policy = pkg.PitchShift()
    draws = policy.draw(B, generator=torch.Generator().manual_seed(5), device=dev).tolist()
    ratios = [policy.ratios[k] for k in draws]
    window = torch.hann_window(n_fft, device=dev)
    mask = torch.arange(T, device=dev)[None, None, :] < lengths[:, None, None]

    def composed():
        out = x.clone()
        for f in set(ratios):
            if f == 1:
                continue
            rows = torch.tensor([b for b in range(B) if ratios[b] == f], device=dev)
            X = torch.stft(x[rows, 0], n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True)
            Y = torch_vocoder(torch, X, 1.0 / float(f), hop)
            s = torch.istft(Y, n_fft, hop, window=window, length=int(round(T * float(f))))
            r, _ = pkg.speed_perturb(s[:, None, :], f, rate, rate)
            n = min(T, r.shape[2])
            out[rows, :, :n] = r[:, :, :n]
        x.copy_(torch.where(mask, out, x))

    ways = {"pitch_shift": lambda: pkg.pitch_shift(x, ratios, rate, lengths, out=x),
            "time_stretch": lambda: pkg.time_stretch(x, ratios, host_lengths),
            "speed_perturb": lambda: pkg.speed_perturb(x, ratios, rate, rate, lengths=host_lengths)}
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T], "n_fft": n_fft,
           "ratios": sorted({str(f) for f in ratios})}
    try:
        composed()
        torch.cuda.synchronize()
        x.copy_(x0)
        ways["torch_composed"] = composed
    except Exception as e:      # (a torch without an FFT for this device: the composition is then not measured)
        doc["torch_composed"] = f"unmeasured: {type(e).__name__}: {e}"[:300]
    ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False, before=dict.fromkeys(ways, lambda: x.copy_(x0)))
    calls = {k: stats(v) for k, v in ms.items()}
    doc["ms_per_call_events_around_reps_calls"] = calls
    if "torch_composed" in calls:
        doc["torch_composed_multiple_of_pitch_shift"] = round(calls["torch_composed"]["median"] / calls["pitch_shift"]["median"], 2)
    doc["time_stretch_share_of_pitch_shift"] = round(calls["time_stretch"]["median"] / calls["pitch_shift"]["median"], 2)
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as f:
                f.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=48000))
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step": step_of(pkg, corpus, torch), "step_pitch": step_of(pkg, corpus, torch, pitch=policy)},
                         args.steps, args.warmup)
            both = {k: stats(v) for k, v in ms.items()}
            doc["step_wall_ms"] = both
            doc["step_pitch_multiple_of_step"] = round(both["step_pitch"]["median"] / both["step"]["median"], 3)
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
