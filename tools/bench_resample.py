"""What crops at a target rate cost per training step: B random crops out of synthetic M4A files (stereo 16-bit at 44.1 kHz,
4096-frame packets, 60 s each), device index tensors and check=False throughout, per shape (B crops of a duration) --
  (a) native       corpus.crops(files, offsets, L) at the files' rate: the path that must not change.  With --parent DIR (a
                   built tree of the parent commit) the same call on the parent's package, alternating with this one
  (b) 16000_mono   corpus.crops(..., sample_rate=16000, mono=True) and
      48000        corpus.crops(..., sample_rate=48000) for the same duration; the resample call alone (HIP events around
                   --reps back-to-back launches over the step's scratch) with its bytes per second from the bytes it reads
                   (the valid source frames) plus those it writes, and the decode pair alone over the same source windows;
                   with --parent the parent's resample call over the same scratch too, alternating with this one
  (c) conv1d       for comparison only, the do-it-yourself route: a native crop of equal duration, then the same filter as a
                   strided torch.nn.functional.conv1d with b output channels (what torchaudio's resample does)
Wall time of a step: torch.cuda.synchronize() in front of and behind it, the ways alternating inside every step, median and
p10 .. p90 of --steps steps after --warmup.  One JSON document, printed and written to --out.
  python tools/bench_resample.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/corpus_resample.json]"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def load_parent(tree):
    """The package of another tree under another name (its own libalacgpu.so next to it)"""
    d = os.path.join(tree, "alac.net_amd")
    spec = importlib.util.spec_from_file_location("alac_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["alac_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def stats(v):
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


def conv1d_resample(torch, table, dev):
    """x [B, C, T] at the source rate -> [B, C, ceil(b T / a)]: every phase an output channel of one strided convolution"""
    a, b, width, d0, w = table
    N = 2 * width + 1
    full = np.zeros((b, 2 * width + a), dtype=np.float32)
    for i in range(b):
        full[i, int(d0[i]) + width:int(d0[i]) + width + N] = w[i]
    kernel = torch.from_numpy(full).to(dev)[:, None, :]

    def run(x):
        B, C_, T = x.shape
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(x.reshape(B * C_, 1, T), (width, width + a)), kernel, stride=a)
        return y.transpose(1, 2).reshape(B, C_, -1)[..., :-(-b * T // a)]

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", action="append", help="BxSECONDS, repeatable (default 64x2 and 256x1)")
    ap.add_argument("--parent", help="a built tree of the parent commit: its crops alternate with this tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corpus_resample.json"))
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth
    from alac.net_amd.resample import device_table, resample_table, source_window
    from bench_corpus import make_file

    synth.build()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rate = 44100
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    blobs = [distinct[f % 2] for f in range(args.files)]
    corpus = pkg.Corpus(blobs)
    parent = load_parent(args.parent).Corpus(blobs) if args.parent else None
    stream = torch.cuda.current_stream(dev)
    results = []
    for B, seconds in [tuple(int(x) for x in s.split("x")) for s in (args.shape or ["64x2", "256x1"])]:
        n_steps = args.steps + args.warmup
        rng = np.random.default_rng(B + seconds)
        files = [torch.from_numpy(rng.integers(0, args.files, B)).to(dev) for _ in range(n_steps)]
        u = [rng.random(B) for _ in range(n_steps)]
        offs = {R: [torch.from_numpy((x * (-(-R * T // rate) - seconds * R + 1)).astype(np.int64)).to(dev) for x in u] for R in (rate, 16000, 48000)}
        L = {R: seconds * R for R in offs}
        tables = {R: device_table(rate, R, dev) for R in (16000, 48000)}
        conv = {R: conv1d_resample(torch, resample_table(rate, R), dev) for R in tables}
        ways = {"native": lambda i: corpus.crops(files[i], offs[rate][i], L[rate], check=False)[0]}
        if parent is not None:
            ways["parent"] = lambda i: parent.crops(files[i], offs[rate][i], L[rate], check=False)[0]
        ways["16000_mono"] = lambda i: corpus.crops(files[i], offs[16000][i], L[16000], check=False, sample_rate=16000, mono=True)[0]
        ways["48000"] = lambda i: corpus.crops(files[i], offs[48000][i], L[48000], check=False, sample_rate=48000)[0]
        ways["conv1d_16000"] = lambda i: conv[16000](corpus.crops(files[i], offs[rate][i], L[rate], check=False)[0])
        ways["conv1d_48000"] = lambda i: conv[48000](corpus.crops(files[i], offs[rate][i], L[rate], check=False)[0])
        if parent is not None:
            assert torch.equal(ways["native"](0), ways["parent"](0)), "the native crops differ from the parent's"
        wall = {m: [] for m in ways}
        for i in range(n_steps):
            for m, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(i)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                del out
                if i >= args.warmup:
                    wall[m].append(dt)
        r = {"crops": B, "seconds": seconds, "wall_ms": {m: stats(v) for m, v in wall.items()}}
        if parent is not None:
            p, n = r["wall_ms"]["parent"], r["wall_ms"]["native"]
            r["native_inside_parent_p10_p90"] = bool(p["p10"] <= n["median"] <= p["p90"])
        # the resample call alone over the last step's scratch, and the decode pair over the same source windows
        for R, mono in ((16000, True), (48000, False)):
            a, b, width, d_d0, d_w = tables[R]
            Ls = source_window(0, L[R], a, b, width)[1]
            out, _ = corpus.crops(files[0], offs[R][0], L[R], check=False, sample_rate=R, mono=mono)
            scratch = corpus._rs_scratch[:B * 2 * Ls].view(B, 2, Ls)
            origin = (torch.div(offs[R][0], b, rounding_mode="floor") * a - width).clamp(min=0)
            valid = (corpus._d_num_frames[files[0]] - origin).clamp(0, Ls)

            def kernel():
                corpus._gpu.resample_device(scratch, B, 2, Ls, origin, valid, offs[R][0], L[R], a, b, width, d_d0, d_w, mono, out,
                                            stream=stream.cuda_stream)

            def decode():
                corpus.crops(files[0], origin, Ls, out=scratch, check=False)

            def parent_kernel():
                parent._gpu.resample_device(scratch, B, 2, Ls, origin, valid, offs[R][0], L[R], a, b, width, d_d0, d_w, mono, theirs,
                                            stream=stream.cuda_stream)

            timed = [("resample_call", kernel, args.reps), ("decode_pair", decode, 1)]
            if parent is not None:
                theirs = torch.empty_like(out)
                parent_kernel()
                assert torch.equal(out, theirs), "the resample call's output differs from the parent's"
                timed.insert(1, ("parent_resample_call", parent_kernel, args.reps))
            ms = {name: [] for name, _, _ in timed}
            for rep in range(args.steps + args.warmup if parent is not None else 30 + 5):
                for name, fn, reps in timed:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(stream)
                    for _ in range(reps):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= (args.warmup if parent is not None else 5):
                        ms[name].append(e0.elapsed_time(e1) / reps)
            moved = int(valid.sum()) * 2 * 4 + out.numel() * 4
            k = stats(ms["resample_call"])
            r[f"{R}{'_mono' if mono else ''}"] = {
                "source_frames_per_crop": Ls, "out_frames": L[R], "table_weights": b * (2 * width + 1), "resample_call_ms": k,
                "bytes_read_plus_written": moved, "resample_call_gb_per_s": round(moved / k["median"] / 1e6, 1),
                "decode_pair_ms_events_around_plan_and_decode": stats(ms["decode_pair"])}
            if parent is not None:
                q = stats(ms["parent_resample_call"])
                r[f"{R}{'_mono' if mono else ''}"].update({"parent_resample_call_ms": q,
                                                           "resample_call_inside_parent_p10_p90": bool(q["p10"] <= k["median"] <= q["p90"])})
        results.append(r)
    doc = {"command": "python tools/bench_resample.py " + " ".join(sys.argv[1:]), "files": args.files, "seconds": args.seconds,
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "blob_mb": round(corpus._blob_bytes / 1e6, 1), "results": results}
    corpus.close()
    if parent is not None:
        parent.close()
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
