"""What crops at a target rate cost per training step: B random crops out of synthetic M4A files (stereo 16-bit at 44.1 kHz,
4096-frame packets, 60 s each), device index tensors and check=False throughout, per shape (B crops of a duration) --
  (a) native       corpus.crops(files, offsets, L) at the files' rate: the path that must not change.  With --parent DIR (a
                   built tree of the parent commit) the same call on the parent's package, alternating with this one
  (b) 16000_mono   corpus.crops(..., sample_rate=16000, mono=True) and
      48000        corpus.crops(..., sample_rate=48000) for the same duration; the resample call alone (_measure.event_ms
                   around --reps back-to-back launches over the step's scratch) with its bytes per second from the bytes it
                   reads (the valid source frames) plus those it writes, and the decode pair alone (one call between the
                   events) over the same source windows, the two alternating inside every repetition, 30 after 5; with
                   --parent the parent's resample call over the same scratch too, alternating with them, --steps after --warmup
  (c) conv1d       for comparison only, the do-it-yourself route: a native crop of equal duration, then the same filter as a
                   strided torch.nn.functional.conv1d with b output channels (what torchaudio's resample does)
Wall time of a step: _measure.wall_ms, median and p10 .. p90.  One JSON document, printed and written to --out.
  python tools/bench_resample.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/corpus_resample.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, inside, load_parent, make_file, stats, wall_ms


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
    ap.add_argument("--shape", action="append", help="BxSECONDS, repeatable (default 64x2 and 256x1)")
    arguments(ap, "corpus_resample.json", reps=20, parent="a built tree of the parent commit: its crops alternate with this tree's")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth
    from alac.net_amd.resample import device_table, resample_table, source_window

    synth.build()
    dev, stream = device(torch)
    rate = 44100
    T = int(args.seconds * rate)
    distinct = [make_file(synth, T, 11 + k) for k in range(2)]
    blobs = [distinct[f % 2] for f in range(args.files)]
    corpus = pkg.Corpus(blobs)
    parent = load_parent(args.parent).Corpus(blobs) if args.parent else None
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
        wall = wall_ms(torch, ways, args.steps, args.warmup)
        r = {"crops": B, "seconds": seconds, "wall_ms": {m: stats(v) for m, v in wall.items()}}
        if parent is not None:
            r["native_inside_parent_p10_p90"] = inside(r["wall_ms"]["parent"], r["wall_ms"]["native"])
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

            timed, reps = {"resample_call": kernel}, {"resample_call": args.reps, "parent_resample_call": args.reps, "decode_pair": 1}
            if parent is not None:
                theirs = torch.empty_like(out)
                parent_kernel()
                assert torch.equal(out, theirs), "the resample call's output differs from the parent's"
                timed["parent_resample_call"] = parent_kernel
            timed["decode_pair"] = decode
            steps, warmup = (args.steps, args.warmup) if parent is not None else (30, 5)
            ms = event_ms(torch, stream, timed, steps, warmup, reps, alternate=True)
            moved = int(valid.sum()) * 2 * 4 + out.numel() * 4
            k = stats(ms["resample_call"])
            r[f"{R}{'_mono' if mono else ''}"] = {
                "source_frames_per_crop": Ls, "out_frames": L[R], "table_weights": b * (2 * width + 1), "resample_call_ms": k,
                "bytes_read_plus_written": moved, "resample_call_gb_per_s": round(moved / k["median"] / 1e6, 1),
                "decode_pair_ms_events_around_plan_and_decode": stats(ms["decode_pair"])}
            if parent is not None:
                q = stats(ms["parent_resample_call"])
                r[f"{R}{'_mono' if mono else ''}"].update({"parent_resample_call_ms": q,
                                                           "resample_call_inside_parent_p10_p90": inside(q, k)})
        results.append(r)
    doc = {"command": command(__file__), "files": args.files, "seconds": args.seconds,
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "blob_mb": round(corpus._blob_bytes / 1e6, 1), "results": results}
    corpus.close()
    if parent is not None:
        parent.close()
    emit(doc, args.out)


if __name__ == "__main__":
    main()
