"""What crops at a target rate cost per training step when the files differ in sample rate: synthetic M4A files (stereo 16-bit,
4096-frame packets, 60 s each), device index tensors and check=False throughout, 64 crops of 2 s --
  (a) single_rate   the step of tools/bench_resample.py on a corpus at 44.1 kHz: crops(..., sample_rate=16000, mono=True) and
                    crops(..., sample_rate=48000).  With --parent DIR (a built tree of the parent commit) the same calls on the
                    parent's package, alternating with this one: this tree's median has to lie inside the parent's p10 .. p90
  (b) mixed         Corpus(half the files at 44.1 kHz, half at 48 kHz, mixed_rates=True): crops(..., sample_rate=16000,
                    mono=True), half the crops from either half, in one call; _measure.event_ms around the plan + decode
                    pair and around the one resample call (--reps back-to-back launches), 30 after 5, one after the other.
                    With --parent the parent's mixed corpus takes the same step, alternating with this one, same criterion
  (c) two_corpora   the two single-rate corpora of the same files and the same crops in two calls of half the batch each
Wall time of a step: _measure.wall_ms, median and p10 .. p90.  One JSON document, printed and written to --out.
  python tools/bench_corpus_mixed.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/corpus_mixed_rates.json]"""
import argparse

import numpy as np

from _measure import arguments, command, device, emit, event_ms, inside, load_parent, make_file, stats, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--crop-seconds", type=int, default=2)
    arguments(ap, "corpus_mixed_rates.json", reps=20,
              parent="a built tree of the parent commit: its single-rate and mixed steps alternate with this tree's")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    synth.build()
    dev, stream = device(torch)
    half, B, R = args.files // 2, args.crops, 16000
    L = args.crop_seconds * R
    rates = (44100, 48000)
    blobs = {r: [make_file(synth, int(args.seconds * r), 11 + k, r) for k in range(2)] for r in rates}
    of_rate = {r: [blobs[r][f % 2] for f in range(half)] for r in rates}
    n_steps = args.steps + args.warmup
    rng = np.random.default_rng(B)
    doc = {"command": command(__file__), "files": args.files, "seconds": args.seconds,
           "crops": B, "crop_seconds": args.crop_seconds, "steps": args.steps, "warmup": args.warmup, "reps": args.reps}

    def measure(ways):
        return {m: stats(v) for m, v in wall_ms(torch, ways, args.steps, args.warmup).items()}

    # (a) the single-rate step, this tree against the parent
    parent_pkg = load_parent(args.parent) if args.parent else None
    single = pkg.Corpus(of_rate[44100] + of_rate[44100])
    parent = parent_pkg.Corpus(of_rate[44100] + of_rate[44100]) if args.parent else None
    T = int(args.seconds * 44100)
    files = [torch.from_numpy(rng.integers(0, 2 * half, B)).to(dev) for _ in range(n_steps)]
    u = [rng.random(B) for _ in range(n_steps)]
    offs = {r: [torch.from_numpy((x * (-(-r * T // 44100) - args.crop_seconds * r + 1)).astype(np.int64)).to(dev) for x in u] for r in (16000, 48000)}
    ways = {}
    for name, c in (("this", single), ("parent", parent)):
        if c is not None:
            ways[f"{name}_16000_mono"] = lambda i, c=c: c.crops(files[i], offs[16000][i], L, check=False, sample_rate=16000, mono=True)[0]
            ways[f"{name}_48000"] = lambda i, c=c: c.crops(files[i], offs[48000][i], args.crop_seconds * 48000, check=False, sample_rate=48000)[0]
    if parent is not None:
        for k in ("16000_mono", "48000"):
            assert torch.equal(ways[f"this_{k}"](0), ways[f"parent_{k}"](0)), "the crops differ from the parent's"
    a = {"wall_ms": measure(ways)}
    if parent is not None:
        for k in ("16000_mono", "48000"):
            a[f"{k}_inside_parent_p10_p90"] = inside(a["wall_ms"][f"parent_{k}"], a["wall_ms"][f"this_{k}"])
        parent.close()
    single.close()
    doc["single_rate"] = a

    # (b) the mixed step and (c) the two single-rate corpora over the same crops
    mixed = pkg.Corpus(of_rate[44100] + of_rate[48000], mixed_rates=True)
    parent = parent_pkg.Corpus(of_rate[44100] + of_rate[48000], mixed_rates=True) if args.parent else None
    two = [pkg.Corpus(of_rate[r]) for r in rates]
    Ty = torch.from_numpy(mixed.resampled_frames(R)).to(dev)
    files = [torch.from_numpy(np.concatenate([rng.integers(0, half, B // 2), half + rng.integers(0, half, B - B // 2)])).to(dev) for _ in range(n_steps)]
    offs = [torch.floor(torch.from_numpy(rng.random(B)).to(dev) * (Ty[f] - L + 1).to(torch.float64)).to(torch.int64) for f in files]
    h = B // 2

    def both(i):
        x = two[0].crops(files[i][:h], offs[i][:h], L, check=False, sample_rate=R, mono=True)[0]
        y = two[1].crops(files[i][h:] - half, offs[i][h:], L, check=False, sample_rate=R, mono=True)[0]
        return x, y

    ways = {"mixed": lambda i: mixed.crops(files[i], offs[i], L, check=False, sample_rate=R, mono=True)[0], "two_corpora": both}
    assert torch.equal(ways["mixed"](0), torch.cat(both(0))), "the mixed crops differ from the single-rate corpora's"
    if parent is not None:
        ways["parent_mixed"] = lambda i: parent.crops(files[i], offs[i], L, check=False, sample_rate=R, mono=True)[0]
        assert torch.equal(ways["mixed"](0), ways["parent_mixed"](0)), "the mixed crops differ from the parent's"
    b = {"wall_ms": measure(ways)}
    if parent is not None:
        b["mixed_inside_parent_p10_p90"] = inside(b["wall_ms"]["parent_mixed"], b["wall_ms"]["mixed"])
        parent.close()
    b["mixed_over_two_corpora"] = round(b["wall_ms"]["mixed"]["median"] / b["wall_ms"]["two_corpora"]["median"], 3)
    # the two halves of the mixed step alone, over the first step's crops
    rt, win = mixed._rate(R), mixed._window(R, L)
    out, _ = mixed.crops(files[0], offs[0], L, check=False, sample_rate=R, mono=True)
    f = files[0]
    kind = rt["d_kind"][f]
    a_, b_, width_, table, _ = rt["d_kinds"][kind].unbind(1)
    origin = (torch.div(offs[0], b_, rounding_mode="floor") * a_ - width_).clamp(min=0)
    Ls, K = win["Ls_max"], win["K"]
    scratch = mixed._rs_scratch[:B * 2 * Ls].view(B, 2, Ls)
    d_files, d_frames, row_table = f.to(torch.int32), win["d_Ls"][kind], table.to(torch.int32)
    valid = mixed._plan_and_decode(d_files, origin, Ls, K, win["S"], scratch, d_frames=d_frames).clone()
    decode = lambda: mixed._plan_and_decode(d_files, origin, Ls, K, win["S"], scratch, d_frames=d_frames)
    kernel = lambda: mixed._gpu.resample_rows_device(scratch, B, 2, Ls, origin, valid, offs[0], L, rt["desc"], rt["d_desc"], rt["d_d0"], rt["d_w"],
                                                     row_table, True, out, stream=stream.cuda_stream)
    moved = int(valid.sum()) * 2 * 4 + out.numel() * 4
    alone = lambda fn, reps: stats(event_ms(torch, stream, {"call": fn}, 30, 5, reps, alternate=False)["call"])
    k = alone(kernel, args.reps)
    b.update({"source_frames_per_crop": {str(r): int(x) for r, x in zip(rates, (win["Ls"][0], win["Ls"][half]))}, "entries_per_crop": K,
              "out_frames": L, "table_weights": [int(d[1] * (2 * d[2] + 1)) for d in rt["desc"]], "resample_call_ms": k,
              "bytes_read_plus_written": moved, "resample_call_gb_per_s": round(moved / k["median"] / 1e6, 1),
              "decode_pair_ms_events_around_plan_and_decode": alone(decode, 1)})
    doc["mixed"] = b
    mixed.close()
    for c in two:
        c.close()
    emit(doc, args.out)


if __name__ == "__main__":
    main()
