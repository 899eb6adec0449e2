"""What Kaldi fbank features cost: the alacgpu_fbank_device call on float32 noise [64, 1, 32000] with KaldiFbank(16000) (window
400, hop 160, 512-point transform, 80 mels) against
  torch_composition  what a user writes today on the same tensor: unfold -> the frame's mean off -> pre-emphasis -> Povey
                     window -> pad to 512 -> rfft -> abs()^2 -> matmul with the mel banks -> clamp(min=2^-23) -> log
  logmel_call        the alacgpu_logmel_device call at n_fft 400, hop 160, 80 mels on the same tensor: the same GEMM shape with
                     K 400 and 201 bins where fbank has 257
_measure.event_ms, the three ways alternating inside every repetition: median and p10 .. p90.  Then the step
corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=..., check=False) with the KaldiFbank against the same
step with LogMel(16000, 400, 160, 80), out of synthetic M4A files (stereo 16-bit at 44.1 kHz, 4096-frame packets):
_measure.wall_ms, the generator seeded with the step in front of either way.  One JSON document, printed and written to --out.
  python tools/bench_fbank.py [--steps 200] [--warmup 20] [--out profiles/fbank.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, make_file, stats, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    arguments(ap, "fbank.json", reps=10)
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    dev, stream = device(torch)
    B, L, R = 64, 32000, 16000
    kaldi, logmel = pkg.KaldiFbank(R), pkg.LogMel(R, 400, 160, 80)
    gpu = pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)])
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, (B, 1, L)).astype(np.float32)).to(dev)
    window, _, fb = kaldi.device_tables(dev)
    out_k = torch.empty((B, 1, 80, kaldi.frames(L)), dtype=torch.float32, device=dev)
    out_l = torch.empty((B, 1, 80, logmel.frames(L)), dtype=torch.float32, device=dev)

    def compose(x):
        """x [B, 1, L] -> [B, 1, n_mels, T']"""
        f = x[:, 0].unfold(1, kaldi.win_length, kaldi.hop_length) * kaldi.scale           # [B, T', 400]
        f = f - f.mean(dim=2, keepdim=True)
        f = f - kaldi.preemphasis * torch.cat([f[..., :1], f[..., :-1]], dim=2)
        f = torch.nn.functional.pad(f * window, (0, kaldi.n_fft - kaldi.win_length))
        p = torch.fft.rfft(f).abs() ** 2                                                  # [B, T', 257]
        return torch.matmul(p, fb.T).clamp(min=2.0 ** -23).log().transpose(1, 2)[:, None]

    calls = {"fbank_call": lambda: kaldi.launch(gpu, x, B, 1, L, L, out_k, stream.cuda_stream),
             "torch_composition": lambda: compose(x),
             "logmel_call": lambda: logmel.launch(gpu, x, B, 1, L, L, out_l, stream.cuda_stream)}
    calls["fbank_call"]()
    worst = float((out_k - compose(x)).abs().max())
    alone = {name: stats(v) for name, v in event_ms(torch, stream, calls, args.steps, args.warmup, args.reps, alternate=True).items()}
    flop = lambda spec, K: 2.0 * B * spec.frames(L) * (K * 2 * spec.n_bins + spec.n_mels * spec.n_bins)
    call = {"tensor": [B, 1, L], "feature_frames": kaldi.frames(L), "max_abs_difference_to_torch_in_ln": round(worst, 6),
            "alone_ms_events_around_reps_calls": alone,
            "fbank_call_tflops": round(flop(kaldi, kaldi.win_length) / alone["fbank_call"]["median"] / 1e9, 2),
            "logmel_call_tflops": round(flop(logmel, logmel.n_fft) / alone["logmel_call"]["median"] / 1e9, 2),
            "fbank_over_logmel": round(alone["fbank_call"]["median"] / alone["logmel_call"]["median"], 3),
            "bins_ratio_257_over_201": round(257 / 201, 3),
            "fbank_median_below_torch_p10": bool(alone["fbank_call"]["median"] < alone["torch_composition"]["p10"])}

    # the step
    rate = 44100
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    corpus = pkg.Corpus([distinct[f % 2] for f in range(args.files)])
    kw = dict(sample_rate=R, mono=True, check=False)
    g = torch.Generator(device=dev)
    ways = {"kaldi_fbank": lambda i: corpus.random_crops(B, L, generator=g, features=kaldi, **kw)[0],
            "log_mel": lambda i: corpus.random_crops(B, L, generator=g, features=logmel, **kw)[0]}
    wall = wall_ms(torch, ways, args.steps, args.warmup, before=g.manual_seed)
    step = {"step": "random_crops(64, 32000, sample_rate=16000, mono=True, features=..., check=False)", "files": args.files,
            "seconds": args.seconds, "wall_ms": {m: stats(v) for m, v in wall.items()}}
    corpus.close()
    gpu.close()
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "kaldi": repr(kaldi), "log_mel": repr(logmel), "call": call, "step": step}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
