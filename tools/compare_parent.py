"""The resampled crops and the resampler's kernels of this tree against the parent commit's, bit for bit, on one GPU --
  crops     both packages in one process (--parent DIR, a built tree of the parent commit): `pcm` and `lengths` of
            the crops of tests/test_corpus_speed.py's files (which are tests/test_corpus_mixed_rates.py's), the first alone and
            all four with mixed_rates=True, resident and tiered (hbm_bytes=0), mono on and off, with given draws of speed= at
            three factors and at the one factor 1, and without speed=; of tests/test_corpus_resample.py's files, stereo and
            mono, at its five (rate, mono) and three lengths; and of random_crops with one seeded generator on both sides,
            with and without speed=.
  kernels   tests/test_resample.py, tests/test_resample_rows.py and tests/test_speed.py run twice in child processes, this
            tree's package over the parent's library (ALACGPU_LIB) and over its own: what every call of the three resample
            entries left in `out` is recorded, and the two records have to be equal call by call.
Every comparison is torch.equal; the first that fails ends the run.  One JSON document with the counts, printed and written to --out.
  python tools/compare_parent.py --parent DIR [--out profiles/crop_pipeline_speed_equal.json]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

from _measure import ROOT, emit, load_parent

sys.path.insert(0, os.path.join(ROOT, "tests"))
ENTRIES = ("resample_device", "resample_rows_device", "resample_ratio_rows_device")
KERNEL_TESTS = ["tests/test_resample.py", "tests/test_resample_rows.py", "tests/test_speed.py"]


def record(path):
    """In a child: the three test files with every `out` of the three entries kept, written to `path`"""
    import pytest
    import torch

    import alac.net_amd as pkg

    kept = []
    for name in ENTRIES:
        def wrapped(self, *args, _inner=getattr(pkg.AlacGpuContext, name), _name=name, **kw):
            r = _inner(self, *args, **kw)
            torch.cuda.synchronize()
            kept.append((_name, args[-1].detach().cpu().clone()))       # (`out` is the last positional argument of all three)
            return r
        setattr(pkg.AlacGpuContext, name, wrapped)
    rc = pytest.main(["-q", "-x", "-p", "no:cacheprovider", *[os.path.join(ROOT, t) for t in KERNEL_TESTS]])
    torch.save(kept, path)
    sys.exit(int(rc))


def crops_of(torch, pkg, speed_paths, resample_files):
    """Every (name, pcm, lengths) of one package, in one fixed order"""
    import test_corpus_mixed_rates as tm
    import test_corpus_resample as tr
    import test_corpus_speed as ts

    got = []
    keep = lambda name, pair: got.append((name, pair[0].clone(), pair[1].clone()))
    dev = lambda v: torch.tensor(v, device="cuda", dtype=torch.int64)
    R, L = ts.TARGET, ts.L
    for files, kw in ((speed_paths[:1], {}), (speed_paths, dict(mixed_rates=True))):
        for tier in ({}, dict(hbm_bytes=0)):
            tag = f"{len(files)} files{' tiered' if tier else ''}"
            with pkg.Corpus(files, **kw, **tier) as corpus:
                for sp in (pkg.SpeedPerturb(), pkg.SpeedPerturb(factors=(1.0,))):
                    cf, co, ck = ts.the_crops(corpus.resampled_frames(R, speed=sp))
                    for mono in (False, True):
                        keep(f"{tag} speed {len(sp.factors)} mono={mono}", corpus.crops(cf, co, L, sample_rate=R, mono=mono, speed=(sp, dev(ck))))
                        keep(f"{tag} speed {len(sp.factors)} mono={mono} device indices",
                             corpus.crops(dev(cf), dev(co), L, sample_rate=R, mono=mono, speed=(sp, dev(ck)), check=False))
                cf, co = tm.the_crops(corpus.resampled_frames(R))
                for mono in (False, True):
                    keep(f"{tag} mono={mono}", corpus.crops(cf, co, L, sample_rate=R, mono=mono))
                for seed in (3, 4):
                    g = torch.Generator(device="cuda").manual_seed(seed)
                    keep(f"{tag} random speed {seed}", corpus.random_crops(16, L, sample_rate=R, mono=True, speed=pkg.SpeedPerturb(), generator=g, check=False))
                    keep(f"{tag} random {seed}", corpus.random_crops(16, L, sample_rate=R, mono=True, generator=g, check=False))
    for stereo, files in resample_files.items():
        for tier in ({}, dict(hbm_bytes=0)):
            rng = np.random.default_rng(6)
            with pkg.Corpus(files, **tier) as corpus:
                for rate, mono in ((16000, True), (48000, False), (16000, False), (22050, True), (44100, True)):
                    Ty = corpus.resampled_frames(rate)
                    for L_ in (1, 700, 5000):
                        crops = [(f, o) for f in range(len(files)) for o in tr.offsets_of(int(Ty[f]), L_, rng)]
                        keep(f"resample stereo={stereo}{' tiered' if tier else ''} {rate} mono={mono} L={L_}",
                             corpus.crops([c[0] for c in crops], [c[1] for c in crops], L_, sample_rate=rate, mono=mono))
                g = torch.Generator(device="cuda").manual_seed(5)
                keep(f"resample stereo={stereo} random", corpus.random_crops(16, 700, sample_rate=16000, mono=True, generator=g, check=False))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built tree of the parent commit")
    ap.add_argument("--record", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_pipeline_speed_equal.json"))
    args = ap.parse_args()
    if args.record:
        record(args.record)
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth
    import test_corpus_resample as tr
    import test_corpus_speed as ts

    synth.build()
    torch.cuda.set_device(0)
    doc = {"command": "python tools/compare_parent.py --parent PARENT   (PARENT: a built checkout of the parent commit; one MI355X)"}
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the kernels: the same tests over either library ----
        lists = {}
        for name, lib in (("parent", os.path.join(args.parent, "alac.net_amd", "csrc", "libalacgpu.so")), ("this", None)):
            env = dict(os.environ, **({"ALACGPU_LIB": lib} if lib else {}))
            path = os.path.join(tmp, name + ".pt")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, f"the kernel tests over the {name} library:\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
            lists[name] = torch.load(path)
        assert [n for n, _ in lists["this"]] == [n for n, _ in lists["parent"]], "the two runs made different calls"
        for i, ((n, x), (_, y)) in enumerate(zip(lists["this"], lists["parent"])):
            assert torch.equal(x, y), f"kernel output {i} ({n}) differs from the parent library's"
        doc["kernel_outputs_equal"] = {n: sum(m == n for m, _ in lists["this"]) for n in ENTRIES}
        # ---- the crops: the two packages side by side ----
        paths = []
        for i, (rate, frames, bits, fl) in enumerate(ts.SPEC):
            paths.append(os.path.join(tmp, f"f{i}_{rate}.m4a"))
            pkg.save(paths[-1], ts.signal(torch, rate, frames, 50 + i), rate, sample_size=bits, frame_length=fl)
        files = {stereo: tr.corpus_files(synth, stereo) for stereo in (True, False)}
        mine, theirs = crops_of(torch, pkg, paths, files), crops_of(torch, load_parent(args.parent), paths, files)
        assert [m[0] for m in mine] == [t[0] for t in theirs]
        for (name, pcm, lengths), (_, pcm_p, lengths_p) in zip(mine, theirs):
            assert torch.equal(pcm, pcm_p) and torch.equal(lengths, lengths_p), f"{name}: differs from the parent's"
        doc.update(crop_calls_equal=len(mine), crop_tensors_equal=2 * len(mine), crops_equal=int(sum(m[1].shape[0] for m in mine)),
                   crop_calls_with_a_nonzero_sample=int(sum(bool(m[1].any()) for m in mine)))
    emit(doc, args.out)


if __name__ == "__main__":
    main()
