"""Encoder throughput: BASELINE cfg2-shaped PCM (4096-frame stereo 16-bit packets from synth.make_pcm, resident on the GPU as
one planar int32 [2, T] tensor) through alacgpu_encode_device at 4096 and 32768 packets.  Each call is timed by device events
around it after a warm-up; the median is reported with Msamples/s (samples = frames x channels) and the compression ratio
(PCM bytes at 16 bits over packet bytes).  For context, the CPU encoder (alac_synth_make_batch: PCM generation + encode, the
same signal, mix weight 1) at --threads threads on the same host.  The output is checked once: every packet decodes back to
its PCM (GPU decoder).  One JSON line per batch size.  Kernel time: run it under rocprofv3 --kernel-trace --stats.
  python tools/bench_encode.py [--packets 4096 32768] [--iters 30] [--warmup 5] [--threads 16]"""
import argparse
import json
import time

import numpy as np

import _measure  # noqa: F401  (the repository root on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU encoder (profiling runs)")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for n in args.packets:
        d, sig, stream_cfgs, _ = synth.config_descs(2, n_packets=n)
        d["mix_weight"] = 1
        b = synth.make_batch(d, sig, n_threads=args.threads, want_pcm=True)          # (the PCM: synth.make_pcm per packet)
        T = n * 4096
        pcm = torch.from_numpy(np.ascontiguousarray(b["pcm"].reshape(T, 2).T)).to(dev)
        first = torch.from_numpy(np.arange(n, dtype=np.int64) * 4096).to(dev)
        frames = torch.full((n,), 4096, dtype=torch.int32, device=dev)
        ci = torch.zeros(n, dtype=torch.int16, device=dev)
        slot = pkg.encode_max_packet_bytes(4096, 16, 2)
        packets = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        sizes = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream()
        times = []
        with pkg.AlacGpuContext(stream_cfgs) as ctx:
            def call():
                ctx.encode_device(pcm, 2, first, frames, ci, n, packets, slot, sizes, st, "planar", T, stream=stream.cuda_stream)

            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            assert (st.cpu() == 0).all()
            # check: the packets decode back to the PCM
            sz = sizes.cpu().numpy().astype(np.int64)
            offs = torch.from_numpy(np.arange(n, dtype=np.int64) * slot).to(dev)
            back = torch.empty((2, T), dtype=torch.int32, device=dev)
            dst = torch.empty(n, dtype=torch.int32, device=dev)
            ctx.decode_into_device(packets, n * slot, offs, sizes, None, n, first, frames, back, 2, "planar", T, None, dst,
                                   stream=stream.cuda_stream)
            torch.cuda.synchronize()
            assert (dst.cpu() == 0).all() and torch.equal(back, pcm), "encoded packets do not decode back to the PCM"
        ms = float(np.median(times))
        out = {"config": 2, "packets": n, "frames_per_packet": 4096, "channels": 2, "iters": args.iters,
               "median_ms": round(ms, 4),
               "spread_ms": [round(float(np.percentile(times, 10)), 4), round(float(np.percentile(times, 90)), 4)],
               "msamples_per_s": round(2 * T / (ms * 1e-3) / 1e6, 1),
               "compression_ratio": round(4 * T / float(sz.sum()), 4),
               "escape_bound_bytes_per_packet": slot}
        if not args.no_cpu:
            reps = []
            for _ in range(3):
                t0 = time.perf_counter()
                c = synth.make_batch(d, sig, n_threads=args.threads)
                reps.append(time.perf_counter() - t0)
            cms = float(np.median(reps)) * 1e3
            out["cpu_make_batch"] = {"threads": args.threads, "median_ms": round(cms, 2),
                                     "msamples_per_s": round(2 * T / (cms * 1e-3) / 1e6, 1),
                                     "compression_ratio": round(4 * T / float(c["sizes"].sum()), 4),
                                     "note": "alac_synth_make_batch: PCM generation + single-mix encode"}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
