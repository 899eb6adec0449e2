"""What Kaldi MFCC features and delta features cost.
(a) the alacgpu_mfcc_device call on float32 noise [64, 1, 32000] with KaldiMfcc(16000) (window 400, hop 160, 512-point
    transform, 23 filters, 13 cepstra) against
      fbank_call         the alacgpu_fbank_device call with 23 filters on the same tensor: the same kernel body without the
                         epilogue, the yardstick
      torch_composition  what a user writes today: that fbank call, then matmul with the DCT and mul with the lifter
(b) the alacgpu_deltas_device call (order 2, window 2, random lengths) on [64, 1, 13, 198] and [64, 1, 80, 198] against its
    torch composition: the clamped index, a gather, conv1d per order, a mask behind the lengths, cat
_measure.event_ms, the ways alternating inside every repetition: median and p10 .. p90.
(c) the step corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=KaldiMfcc(16000), deltas=Deltas(),
    check=False) against the same step with features=KaldiFbank(16000, n_mels=23), out of synthetic M4A files (stereo 16-bit
    at 44.1 kHz, 4096-frame packets): _measure.wall_ms, the generator seeded with the step in front of either way.
One JSON document, printed and written to --out.
  python tools/bench_mfcc.py [--steps 200] [--warmup 20] [--out profiles/mfcc.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, make_file, stats, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    arguments(ap, "mfcc.json", reps=10)
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    dev, stream = device(torch)
    B, L, R = 64, 32000, 16000
    mfcc, fbank, deltas = pkg.KaldiMfcc(R), pkg.KaldiFbank(R, n_mels=23), pkg.Deltas()
    gpu = pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)])
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, 1, L)).astype(np.float32)).to(dev)
    dct, lifter = mfcc.device_tables(dev)[3:]
    Tf = mfcc.frames(L)
    out_m = torch.empty((B, 1, 13, Tf), dtype=torch.float32, device=dev)
    out_f = torch.empty((B, 1, 23, Tf), dtype=torch.float32, device=dev)

    def compose(x):
        fbank.launch(gpu, x, B, 1, L, L, out_f, stream.cuda_stream)
        return torch.matmul(dct, out_f) * lifter[:, None]

    calls = {"mfcc_call": lambda: mfcc.launch(gpu, x, B, 1, L, L, out_m, stream.cuda_stream),
             "fbank_call": lambda: fbank.launch(gpu, x, B, 1, L, L, out_f, stream.cuda_stream),
             "torch_composition": lambda: compose(x)}
    calls["mfcc_call"]()
    worst = float((out_m - compose(x)).abs().max())
    alone = {name: stats(v) for name, v in event_ms(torch, stream, calls, args.steps, args.warmup, args.reps, alternate=True).items()}
    call = {"tensor": [B, 1, L], "feature_frames": Tf, "max_abs_difference_to_torch": round(worst, 6),
            "alone_ms_events_around_reps_calls": alone,
            "mfcc_over_fbank": round(alone["mfcc_call"]["median"] / alone["fbank_call"]["median"], 4),
            "mfcc_median_above_fbank_p90_by": round(max(alone["mfcc_call"]["median"] / alone["fbank_call"]["p90"] - 1.0, 0.0), 4),
            "mfcc_median_below_torch_p10": bool(alone["mfcc_call"]["median"] < alone["torch_composition"]["p10"])}

    # the delta call
    W, order = deltas.window, deltas.order
    first = torch.arange(-W, W + 1, dtype=torch.float32, device=dev) / (2.0 * sum(j * j for j in range(1, W + 1)))

    def compose_deltas(f, lens):
        """f [B, 1, F, T], lens [B] -> [B, 1, (order + 1) F, T]: Kaldi's clamp into the features per order"""
        Bf, _, F, T = f.shape
        n = lens.clamp(0, T)
        blocks, kernel = [f], torch.ones(1, device=dev)
        t = torch.arange(T, device=dev)
        for k in range(1, order + 1):
            kernel = torch.nn.functional.conv1d(kernel.view(1, 1, -1), first.flip(0).view(1, 1, -1), padding=2 * W).view(-1)
            idx = (t[None, :, None] + torch.arange(-k * W, k * W + 1, device=dev)[None, None, :]).clamp(min=0)
            idx = torch.minimum(idx, (n - 1).clamp(min=0)[:, None, None])                      # [B, T, taps]
            g = torch.gather(f[:, 0, :, None, :].expand(Bf, F, T, T), 3, idx[:, None].expand(Bf, F, T, idx.shape[2]))
            blocks.append(((g * kernel).sum(dim=3) * (t[None, :] < n[:, None])[:, None, :])[:, None])
        return torch.cat(blocks, dim=2)

    delta_calls = {}
    for F in (13, 80):
        f = torch.from_numpy(rng.standard_normal((B, 1, F, Tf)).astype(np.float32)).to(dev)
        lens = torch.from_numpy(rng.integers(Tf // 2, Tf + 1, B)).to(dev)
        out_d = torch.empty((B, 1, deltas.lines(F), Tf), dtype=torch.float32, device=dev)
        scales = deltas.device_scales(dev)
        ways = {"deltas_call": lambda f=f, lens=lens, out_d=out_d: gpu.deltas_device(f, out_d, B, 1, F, Tf, Tf, Tf, lens, order, W, scales,
                                                                                     stream=stream.cuda_stream),
                "torch_composition": lambda f=f, lens=lens: compose_deltas(f, lens)}
        ways["deltas_call"]()
        worst_d = float((out_d - compose_deltas(f, lens)).abs().max())
        ms = {name: stats(v) for name, v in event_ms(torch, stream, ways, args.steps, args.warmup, args.reps, alternate=True).items()}
        gb = 4.0 * B * F * Tf * (order + 2) / 1e9
        delta_calls[f"[{B}, 1, {F}, {Tf}]"] = {
            "max_abs_difference_to_torch": round(worst_d, 7), "alone_ms_events_around_reps_calls": ms,
            "deltas_call_gb_per_s": round(gb / (ms["deltas_call"]["median"] / 1e3), 1),
            "deltas_median_below_torch_p10": bool(ms["deltas_call"]["median"] < ms["torch_composition"]["p10"])}

    # the step
    rate = 44100
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    corpus = pkg.Corpus([distinct[f % 2] for f in range(args.files)])
    kw = dict(sample_rate=R, mono=True, check=False)
    g = torch.Generator(device=dev)
    ways = {"kaldi_mfcc_deltas": lambda i: corpus.random_crops(B, L, generator=g, features=mfcc, deltas=deltas, **kw)[0],
            "kaldi_fbank_23": lambda i: corpus.random_crops(B, L, generator=g, features=fbank, **kw)[0]}
    wall = wall_ms(torch, ways, args.steps, args.warmup, before=g.manual_seed)
    step = {"step": "random_crops(64, 32000, sample_rate=16000, mono=True, features=..., [deltas=Deltas(),] check=False)",
            "files": args.files, "seconds": args.seconds, "wall_ms": {m: stats(v) for m, v in wall.items()}}
    corpus.close()
    gpu.close()
    doc = {"command": command(__file__), "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "mfcc": repr(mfcc),
           "fbank": repr(fbank), "deltas": repr(deltas), "call": call, "delta_call": delta_calls, "step": step}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
