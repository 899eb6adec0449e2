"""What a window is worth: random crops of synthetic M4A files (stereo 16-bit, 4096-frame packets) decoded by ONE windowed
load_batch (frame_offsets= and max_frames=: only the packets that overlap a crop are uploaded and decoded) against the way
without windows -- load_batch of the whole files, then a gather of the crops out of the [F, C, T] tensor.  The two alternate
inside every round; per round the wall time of the whole call (parse, upload, decode, gather) and the kernel time (device
events around the decode call) are taken, and the medians reported.  The crops are checked equal once.  One JSON line.
  python tools/bench_load_window.py [--files 128] [--seconds 180] [--crop 2.0] [--rounds 3] [--distinct 2]"""
import argparse
import json
import time

import numpy as np

from _measure import make_file


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--crop", type=float, default=2.0, help="crop length in seconds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=2, help="distinct files behind the sources (the bytes are shared)")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    torch.cuda.set_device(0)
    T = int(args.seconds * 44100)
    crop = int(args.crop * 44100)
    files = [make_file(synth, T, 11 + k) for k in range(args.distinct)]
    sources = [files[f % len(files)] for f in range(args.files)]
    assert pkg.info(sources[0])["num_frames"] == T
    rng = np.random.default_rng(1)

    # kernel time: device events around every decode call (the windowed and the whole-file load_batch make one each)
    kernel_ms = []
    plain = pkg.AlacGpuContext.decode_window_into_device

    def timed(self, *a, **kw):
        stream = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        plain(self, *a, **kw)
        e1.record(stream)
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))

    pkg.AlacGpuContext.decode_window_into_device = timed

    def windowed(offs):
        out, lengths, _ = pkg.load_batch(sources, frame_offsets=offs, max_frames=crop)
        torch.cuda.synchronize()
        return out

    def full_then_gather(offs):
        full, lengths, _ = pkg.load_batch(sources)
        idx = torch.from_numpy(offs).to(full.device)[:, None] + torch.arange(crop, device=full.device)[None, :]
        out = torch.gather(full, 2, idx[:, None, :].expand(-1, full.shape[1], -1))
        del full
        torch.cuda.synchronize()
        return out

    modes = {"windowed": windowed, "full_then_gather": full_then_gather}
    wall = {m: [] for m in modes}
    kern = {m: [] for m in modes}
    for r in range(args.rounds + 1):                      # round 0: warm-up and the equality check
        offs = rng.integers(0, T - crop + 1, args.files).astype(np.int64)
        outs = {}
        for m, fn in modes.items():
            kernel_ms.clear()
            t0 = time.perf_counter()
            outs[m] = fn(offs)
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                wall[m].append(dt)
                kern[m].append(sum(kernel_ms))
        if r == 0:
            assert torch.equal(outs["windowed"], outs["full_then_gather"]), "the crops differ"
        del outs
        torch.cuda.empty_cache()
    med = lambda v: round(float(np.median(v)), 3)
    print(json.dumps({"files": args.files, "seconds": args.seconds, "crop_frames": crop, "rounds": args.rounds,
                      "kernel_ms": {m: med(v) for m, v in kern.items()}, "wall_ms": {m: med(v) for m, v in wall.items()},
                      "kernel_speedup": round(med(kern["full_then_gather"]) / med(kern["windowed"]), 1),
                      "wall_speedup": round(med(wall["full_then_gather"]) / med(wall["windowed"]), 2)}), flush=True)


if __name__ == "__main__":
    main()
