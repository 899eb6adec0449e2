"""What building a resident corpus from PCM on the GPU costs, against the routes it replaces.  Every measurement runs in a child
process of its own (memory peaks are compared: one configuration per process), after a warm-up, medians over --steps steps:
  compact   cfg2-shaped PCM (4096-frame stereo 16-bit packets) at 4096 and 32768 packets, encoded once into slots; then
            alacgpu_compact_packets_device (HIP events around the call) against the torch gather the parent commit compacted
            with (repeat_interleave / arange / index, the tail of its _encode_tensor) on the same slot buffer: time and
            torch.cuda.max_memory_allocated over the slots.  Also the encode's time, the compaction's share of encode +
            compact and its bytes read plus written over time as a fraction of --peak-tbs TB/s.  The two blobs are compared.
  build     wall time from PCM on the device to the first crops result (32 files of 60 s stereo): Corpus.from_pcm against
            save_batch to memory and Corpus(files).
  save      save_batch's wall time with the compaction kernel and with the parent's gather patched in.
One JSON line.
  python tools/bench_corpus_build.py [--steps 15] [--warmup 3] [--files 32] [--seconds 60]"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cfg2_pcm(torch, n, threads=16):
    from alac.net_amd import synth

    d, sig, _, _ = synth.config_descs(2, n_packets=n)
    d["mix_weight"] = 1
    b = synth.make_batch(d, sig, n_threads=threads, want_pcm=True)
    return torch.from_numpy(np.ascontiguousarray(b["pcm"].reshape(n * 4096, 2).T)).cuda()


def gather(torch, d_packets, d_sizes, slot):
    """The parent commit's compaction: a gather of every packet's bytes with int64 index arrays of the blob's length"""
    n, dev = d_sizes.shape[0], d_sizes.device
    sizes64 = d_sizes.to(torch.int64)
    ends = torch.cumsum(sizes64, 0)
    total = int(ends[-1])
    starts = ends - sizes64
    owner = torch.repeat_interleave(torch.arange(n, device=dev), sizes64, output_size=total)
    src_idx = owner * slot + (torch.arange(total, device=dev) - starts[owner])
    return d_packets[src_idx]


def encode_tensor_gather(pcm, lengths, sample_size, frame_length, device):
    """The parent commit's _encode_tensor (save / save_batch): encode, read the statuses, gather, copy"""
    import torch

    import alac.net_amd as pkg

    F, C_, T = pcm.shape
    with pkg.AlacGpuContext([(frame_length, sample_size, 40, 10, 14, C_)], device) as ctx:
        e = pkg._encode_slots(ctx, pcm, lengths, frame_length, torch.cuda.current_stream(pcm.device).cuda_stream)
        st = e.d_st.cpu().numpy()
    assert (st == 0).all()
    blob = gather(torch, e.d_packets, e.d_sizes, e.slot).cpu().numpy().tobytes()
    sizes = e.d_sizes.cpu().numpy().astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    out, p = [], 0
    for f in range(F):
        out.append([blob[offs[q]:offs[q + 1]] for q in range(p, p + e.counts[f])])
        p += e.counts[f]
    return out, [e.frames[e.file_of == f] for f in range(F)]


def median_spread(times):
    return {"median_ms": round(float(np.median(times)), 4),
            "p10_p90_ms": [round(float(np.percentile(times, 10)), 4), round(float(np.percentile(times, 90)), 4)]}


def child_compact(args):
    import torch

    import alac.net_amd as pkg

    n, way = args.packets, args.way
    dev = torch.device("cuda", 0)
    pcm = cfg2_pcm(torch, n).unsqueeze(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"packets": n, "way": way}
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], 0) as ctx:
        enc = []
        for i in range(args.warmup + args.steps):
            e = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e = pkg._encode_slots(ctx, pcm, [n * 4096], 4096, stream)
            e1.record()
            e1.synchronize()
            enc.append(e0.elapsed_time(e1))
        out["encode"] = median_spread(enc[args.warmup:])
        assert bool((e.d_st == 0).all())
        total = int(e.d_sizes.sum())
        out["packet_bytes"] = total
        del pcm
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        times = []
        if way == "kernel":
            d_blob = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
            d_off = torch.empty(n, dtype=torch.int64, device=dev)
            d_total = torch.zeros(1, dtype=torch.int64, device=dev)
            for i in range(args.warmup + args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.compact_packets_device(e.d_packets, e.slot, e.d_sizes, n, d_blob, 0, total, d_off, d_total, stream=stream)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            assert int(d_total[0]) == total
            blob = d_blob[:total]
        else:
            for i in range(args.warmup + args.steps):
                blob = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                blob = gather(torch, e.d_packets, e.d_sizes, e.slot)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
        out["compact"] = median_spread(times[args.warmup:])
        out["peak_bytes_over_slots_and_sizes"] = int(torch.cuda.max_memory_allocated() - base)
        ms = out["compact"]["median_ms"]
        moved = 2 * total + 12 * n + 8 * n       # the packets read and written, the sizes (twice) and the offsets
        out["fraction_of_peak_bandwidth"] = round(moved / (ms * 1e-3) / (args.peak_tbs * 1e12), 4)
        out["share_of_encode_plus_compact"] = round(ms / (ms + out["encode"]["median_ms"]), 4)
        # one checksum both ways must agree on: the blob's bytes, weighted by position
        w = torch.arange(total, device=dev, dtype=torch.int64) % 65521 + 1
        out["checksum"] = int((blob.to(torch.int64) * w).sum())
    print(json.dumps(out), flush=True)


def tone(torch, F, T, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float32)
    w = torch.rand((F, 2, 1), generator=g, device="cuda") * 0.05 + 0.01
    x = 9000 * torch.sin(t * w) + 3000 * torch.sin(t * w * 3.7) + 40 * torch.randn((F, 2, T), generator=g, device="cuda")
    return x.to(torch.int32)


def child_build(args):
    import torch

    import alac.net_amd as pkg

    F, T = args.files, int(args.seconds * 44100)
    pcm = tone(torch, F, T, 5)
    lengths = [T] * F
    crops = (list(range(F)), [1000] * F, 44100)

    def from_pcm():
        with pkg.Corpus.from_pcm(pcm, lengths, 44100) as c:
            out, _ = c.crops(*crops, dtype=torch.int32)
            torch.cuda.synchronize()
            return out

    def files():
        bufs = [io.BytesIO() for _ in range(F)]
        pkg.save_batch(bufs, pcm, lengths, 44100)
        with pkg.Corpus([b.getvalue() for b in bufs]) as c:
            out, _ = c.crops(*crops, dtype=torch.int32)
            torch.cuda.synchronize()
            return out

    way = from_pcm if args.way == "from_pcm" else files
    times = []
    for i in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = way()
        times.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out, pcm[:, :, 1000:1000 + 44100])
    print(json.dumps({"way": args.way, "files": F, "seconds": args.seconds, **median_spread(times[args.warmup:])}), flush=True)


def child_save(args):
    import torch

    import alac.net_amd as pkg

    if args.way == "gather":
        pkg._encode_tensor = encode_tensor_gather
    F, T = args.files, int(args.seconds * 44100)
    pcm = tone(torch, F, T, 5)
    lengths = [T] * F
    times = []
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for i in range(args.warmup + args.steps):
        bufs = [io.BytesIO() for _ in range(F)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sizes = pkg.save_batch(bufs, pcm, lengths, 44100)
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"way": args.way, "files": F, "seconds": args.seconds, "file_bytes": int(sum(sizes)),
                      "peak_bytes_over_pcm": int(torch.cuda.max_memory_allocated() - base), **median_spread(times[args.warmup:])}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM peak the copy's traffic is set against, TB/s")
    ap.add_argument("--child", choices=["compact", "build", "save"])
    ap.add_argument("--way")
    ap.add_argument("--packets", type=int, default=4096)
    args = ap.parse_args()
    if args.child:
        return {"compact": child_compact, "build": child_build, "save": child_save}[args.child](args)
    from alac.net_amd import synth

    synth.build()

    def run(child, way, *more):      # a fresh process per configuration, one at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--way", way, "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--files", str(args.files), "--seconds", str(args.seconds), "--peak-tbs", str(args.peak_tbs), *more]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"steps": args.steps, "warmup": args.warmup, "compact": [], "build": {}, "save_batch": {}}
    for n in (4096, 32768):
        k, g = run("compact", "kernel", "--packets", str(n)), run("compact", "gather", "--packets", str(n))
        assert k["checksum"] == g["checksum"] and k["packet_bytes"] == g["packet_bytes"], "the two compactions differ"
        out["compact"].append({"packets": n, "packet_bytes": k["packet_bytes"], "kernel": k, "parent_gather": g,
                               "speedup": round(g["compact"]["median_ms"] / k["compact"]["median_ms"], 2)})
    for way in ("from_pcm", "files"):
        out["build"][way] = run("build", way)
    for way in ("kernel", "gather"):
        out["save_batch"][way] = run("save", way)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
