"""Kernel time of the destination mode against the slot layout: BASELINE cfg2 (4096-frame stereo 16-bit packets) at 4096 and
32768 packets, alacgpu_decode_batch_device (int32 slots) next to alacgpu_decode_into_device in all four dtype x layout
combinations (gap-free [C, T] / [T, C] tensor).  The modes alternate inside every round (drift and neighbours' load cancel),
each call is timed by device events around it, after a warm-up of every mode; the median per mode is reported, and every
output is checked against the slot layout's once.  One JSON line per batch size.
  python tools/bench_decode_into.py [--packets 4096 32768] [--rounds 30] [--warmup 5]"""
import argparse
import json

import numpy as np

import _measure  # noqa: F401  (the repository root on sys.path)

MODES = ["slots_int32", "int32_interleaved", "int32_planar", "float32_interleaved", "float32_planar"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for n in args.packets:
        b = synth.make_config_batch(2, n_packets=n)
        nb = int(b["blob"].size)
        blob = torch.zeros((nb + 63) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
        blob[:nb] = torch.from_numpy(b["blob"]).to(dev)
        off = torch.from_numpy(b["offsets"].astype(np.int64)).to(dev)
        sz = torch.from_numpy(b["sizes"].astype(np.int32)).to(dev)
        frames = np.full(n, 4096, dtype=np.int64)
        T = int(frames.sum())
        first = torch.from_numpy(np.arange(n, dtype=np.int64) * 4096).to(dev)
        d_frames = torch.from_numpy(frames.astype(np.int32)).to(dev)
        slot = 2 * 4096
        pcm = torch.empty((n, slot), dtype=torch.int32, device=dev)
        outs = {"int32": torch.empty(2 * T, dtype=torch.int32, device=dev),
                "float32": torch.empty(2 * T, dtype=torch.float32, device=dev)}
        os_ = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream()
        times = {m: [] for m in MODES}
        with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
            def call(m):
                if m == "slots_int32":
                    ctx.decode_batch_device(blob, nb, off, sz, None, n, pcm, slot, None, os_, st, stream=stream.cuda_stream)
                else:
                    dt, lay = m.split("_")
                    ctx.decode_into_device(blob, nb, off, sz, None, n, first, d_frames, outs[dt], 2, lay,
                                           T if lay == "planar" else 0, os_, st, stream=stream.cuda_stream)

            for m in MODES:                       # warm-up (code objects, the parking place, the flag arrays)
                for _ in range(args.warmup):
                    call(m)
            torch.cuda.synchronize()
            # results: every mode equals the slot layout
            call("slots_int32")
            ref = pcm.view(n, 4096, 2).cpu()
            for m in MODES[1:]:
                call(m)
                dt, lay = m.split("_")
                got = outs[dt].cpu()
                want = ref.reshape(T, 2)
                if lay == "planar":
                    want = want.T.contiguous()
                want = want.reshape(-1)
                if dt == "float32":
                    want = want.to(torch.float32) * 2.0 ** -15
                assert torch.equal(got, want), m
                assert (st.cpu() == 0).all(), m
            for _ in range(args.rounds):
                for m in MODES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call(m)
                    e1.record(stream)
                    e1.synchronize()
                    times[m].append(e0.elapsed_time(e1))
        med = {m: float(np.median(times[m])) for m in MODES}
        base = med["slots_int32"]
        print(json.dumps({"config": 2, "packets": n, "rounds": args.rounds, "median_ms": {m: round(v, 4) for m, v in med.items()},
                          "vs_slots": {m: round(med[m] / base - 1.0, 4) for m in MODES[1:]},
                          "spread_ms": {m: [round(float(np.percentile(times[m], 10)), 4), round(float(np.percentile(times[m], 90)), 4)]
                                        for m in MODES}}), flush=True)


if __name__ == "__main__":
    main()
