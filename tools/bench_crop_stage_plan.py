"""What the host side of a crop step costs against the parent commit: two steps on this tree's package and on the parent's in one
process, the four ways in turn inside every step (_measure.wall_ms: the host's work, the enqueues and the device's work) --
  features     corpus.random_crops(64, 32000, sample_rate=16000, mono=True, features=KaldiFbank(16000), check=False)
  all_draws    the same with speed=SpeedPerturb(), mix=AddNoise(the corpus itself, (5, 20)), reverb=Reverb(4 files of 2 s,
               max_seconds=0.5), effects=Effects.telephone() and augment=SpecAugment(): every stage that draws
out of 8 files of 8 s stereo 16-bit at 48 kHz.  The kernels are the same on both sides, so only host time can differ.  Per step
"each_median_inside_the_others_p10_p90": whether each side's median lies inside the other side's p10 .. p90.  Without --parent
only this tree is timed.  One JSON document, printed and written to --out.
  python tools/bench_crop_stage_plan.py [--parent DIR] [--steps 200] [--warmup 20] [--out profiles/crop_stage_plan.json]"""
import argparse

from _measure import arguments, device, emit, inside, load_parent, make_file, stats, wall_ms

B, L, R = 64, 32000, 16000


def steps(p, corpus, rirs, torch):
    spec = p.KaldiFbank(R)
    kw = dict(sample_rate=R, mono=True, features=spec, check=False)
    draws = dict(speed=p.SpeedPerturb(), mix=p.AddNoise(corpus, (5, 20)), reverb=p.Reverb(rirs, max_seconds=0.5),
                 effects=p.Effects.telephone(), augment=p.SpecAugment())
    g = torch.Generator().manual_seed(3)
    return {"features": lambda i: corpus.random_crops(B, L, generator=g, **kw)[0],
            "all_draws": lambda i: corpus.random_crops(B, L, generator=g, **draws, **kw)[0]}


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "crop_stage_plan.json", parent="a built tree of the parent commit: both steps are timed on both packages")
    args = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    device(torch)
    synth.build()
    blobs = [make_file(synth, 384000 + 4321 * i, 20 + i, rate=48000) for i in range(8)]
    rir_files = [make_file(synth, 2 * 44100, 31 + k) for k in range(4)]
    sides = {"this": pkg}
    if args.parent:
        sides["parent"] = load_parent(args.parent)
    corpora = {side: (p.Corpus(blobs), p.Corpus(rir_files)) for side, p in sides.items()}
    ways = {f"{side}_{step}": fn for side, p in sides.items() for step, fn in steps(p, *corpora[side], torch).items()}
    wall = {way: stats(v) for way, v in wall_ms(torch, ways, args.steps, args.warmup).items()}
    shown = f"python tools/bench_crop_stage_plan.py --steps {args.steps} --warmup {args.warmup}"     # (neither where the parent's tree lay nor --out)
    doc = {"command": shown, "steps": args.steps, "warmup": args.warmup, "wall_ms": wall}
    if args.parent:
        doc["command"] += " --parent PARENT   (PARENT: a built checkout of the parent commit; one MI355X)"
        doc["each_median_inside_the_others_p10_p90"] = {
            step: inside(wall["parent_" + step], wall["this_" + step]) and inside(wall["this_" + step], wall["parent_" + step])
            for step in ("features", "all_draws")}
    for pair in corpora.values():
        for c in pair:
            c.close()
    emit(doc, args.out)


if __name__ == "__main__":
    main()
