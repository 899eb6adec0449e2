"""What the STFT stage costs --
  call      spectrogram(x, Spectrogram(...)) on [64, 1, 44100] at (22050, 1024, 256) and (22050, 2048, 512): power 2, the
            complex spectrum, and a mel filterbank (80 lines at 1024, 128 at 2048) with log="ln"; against the torch
            composition on the same tensor (torch.stft, abs^2, matmul, clamp, log -- as far as the kind goes) and against
            log_mel with the same mel configuration.  The speech shape [64, 1, 32000] at (16000, 512, 160) with 80 mels,
            against log_mel with LogMel(16000, 400, 160, 80).  _measure.event_ms, one way after the other: median and
            p10 .. p90 of the time per call.
  step      corpus.random_crops(64, 44100, sample_rate=22050, mono=True, features=..., check=False) with the mel Spectrogram
            (2048, 512, 128), with the LogMel of the same shape and with no features (_measure.wall_ms, the ways in turn), and
            with --parent DIR (a built tree of the parent commit) the LogMel step by this tree's package and by the parent's, in
            turn: "unchanged_step_overlaps_parent" is whether their p10 .. p90 ranges overlap.  Without --parent: "unmeasured".
One JSON document, printed and written to --out.
  python tools/bench_stft.py [--steps 100] [--warmup 10] [--parent DIR] [--out profiles/stft.json]"""
import argparse
import os
import tempfile

import numpy as np

from _measure import arguments, command, device, emit, event_ms, load_parent, make_file, stats, wall_ms

B, T, RATE = 64, 44100, 22050


def step_of(pkg, corpus, torch, features):
    g = torch.Generator().manual_seed(3)
    kw = {} if features is None else dict(features=features)
    return lambda i: corpus.random_crops(B, T, generator=g, sample_rate=RATE, mono=True, check=False, **kw)


def overlap(a, b):
    return bool(a["p10"] <= b["p90"] and b["p10"] <= a["p90"])


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "stft.json", reps=5, parent="a built tree of the parent commit: the unchanged LogMel step is timed on both")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev, stream = device(torch)
    rng = np.random.default_rng(1)
    x = torch.from_numpy((0.3 * rng.standard_normal((B, 1, T))).astype(np.float32)).to(dev)
    speech = torch.from_numpy((0.3 * rng.standard_normal((B, 1, 32000))).astype(np.float32)).to(dev)
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shape": [B, 1, T],
           "speech_shape": [B, 1, 32000], "ms_per_call_events_around_reps_calls": {}, "call_median_below_torch_p10": {},
           "largest_difference_from_the_composition": {}}

    def composition(sig, n_fft, hop, window, fb, log):
        def run():
            z = torch.stft(sig[:, 0], n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True)
            if fb is None and not log:
                return z
            p = z.real ** 2 + z.imag ** 2
            if fb is not None:
                p = torch.matmul(fb, p)
            return torch.log(p.clamp(min=1e-10)) if log else p
        return run

    def measure(tag, sig, rate, n_fft, hop, n_mels, logmel):
        window = torch.from_numpy(np.array(pkg.Spectrogram(rate, n_fft, hop).window)).to(dev)
        fb = pkg.mel_filterbank(rate, n_fft, n_mels)
        d_fb = torch.from_numpy(fb).to(dev)
        kinds = {"power": (pkg.Spectrogram(rate, n_fft, hop), composition(sig, n_fft, hop, window, None, False)),
                 "complex": (pkg.Spectrogram(rate, n_fft, hop, power=None), composition(sig, n_fft, hop, window, None, False)),
                 f"mel{n_mels}_ln": (pkg.Spectrogram(rate, n_fft, hop, filterbank=fb, log="ln"), composition(sig, n_fft, hop, window, d_fb, True))}
        ways = {}
        for kind, (spec, torch_way) in kinds.items():
            ways[f"{kind}.spectrogram"] = lambda spec=spec: pkg.spectrogram(sig, spec)
            ways[f"{kind}.torch"] = torch_way
        ways[f"mel{n_mels}_ln.log_mel"] = lambda: pkg.log_mel(sig, logmel)
        mel_spec, mel_torch = kinds[f"mel{n_mels}_ln"]
        doc["largest_difference_from_the_composition"][tag] = float((pkg.spectrogram(sig, mel_spec)[:, 0] - mel_torch()).abs().max())
        ms = event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=False)
        calls = {k: stats(v) for k, v in ms.items()}
        doc["ms_per_call_events_around_reps_calls"][tag] = calls
        doc["call_median_below_torch_p10"][tag] = {kind: bool(calls[f"{kind}.spectrogram"]["median"] < calls[f"{kind}.torch"]["p10"]) for kind in kinds}

    measure("22050_1024_256", x, RATE, 1024, 256, 80, pkg.LogMel(RATE, 1024, 256, 80))
    measure("22050_2048_512", x, RATE, 2048, 512, 128, pkg.LogMel(RATE, 2048, 512, 128))
    measure("16000_512_160_speech", speech, 16000, 512, 160, 80, pkg.LogMel(16000, 400, 160, 80))
    doc["unmeasured"] = ["counters (rocprofv3 --pmc): LDS bank conflicts of the digit-reversed reads", "n_fft 256", "two channels",
                         "hops other than n_fft / 4 and 160", "power 1"]
    synth.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(8):
            paths.append(os.path.join(tmp, f"f{i}.m4a"))
            with open(paths[-1], "wb") as fh:
                fh.write(make_file(synth, 400000 + 4321 * i, 20 + i, rate=44100))
        mel = lambda p: p.LogMel(RATE, 2048, 512, 128)
        spec = pkg.Spectrogram(RATE, 2048, 512, filterbank=pkg.mel_filterbank(RATE, 2048, 128), log="ln")
        with pkg.Corpus(paths) as corpus:
            ms = wall_ms(torch, {"step_spectrogram_mel": step_of(pkg, corpus, torch, spec), "step_logmel": step_of(pkg, corpus, torch, mel(pkg)),
                                 "step_pcm": step_of(pkg, corpus, torch, None)}, args.steps, args.warmup)
            doc["step_wall_ms"] = {k: stats(v) for k, v in ms.items()}
            doc["unchanged_step_overlaps_parent"] = "unmeasured"
            if args.parent:
                parent = load_parent(args.parent)
                with parent.Corpus(paths) as theirs:
                    ms = wall_ms(torch, {"this": step_of(pkg, corpus, torch, mel(pkg)), "parent": step_of(parent, theirs, torch, mel(parent))},
                                 args.steps, args.warmup)
                    both = {k: stats(v) for k, v in ms.items()}
                    doc["unchanged_step_wall_ms"] = both
                    doc["unchanged_step_overlaps_parent"] = overlap(both["this"], both["parent"])
    emit(doc, args.out)


if __name__ == "__main__":
    main()
