"""What the benchmark tools share: the two timing methods, the statistics, the verdict against the parent and a tool's frame.
Importing it puts the repository root and tools/ on sys.path, as every tool needs.

  event_ms   the time of a call on the device.  Per repetition: before[way]() if there is one, two HIP events made,
             torch.cuda.synchronize(), the first event recorded on the stream, `reps` back-to-back calls, the second event
             recorded, and a wait for it.  Inside the events is nothing but the calls: their enqueue on the host where the device
             is faster than the host, their work on the device where it is not.  `before`, the events' making and the synchronize
             are outside.  The first `warmup` repetitions of every way are run and discarded, `steps` are kept, and a kept value
             is the time between the events divided by `reps`: milliseconds per call.  With alternate=False a way runs all
             its repetitions before the next way starts (clocks and caches settle on one way; drift during the run hits the
             ways differently); with alternate=True the ways take turns inside every repetition (drift hits them alike; each
             starts on what the other left in the caches).  A tool says which at its call.
  wall_ms    the time of a training step as the host sees it.  Per step and way: torch.cuda.synchronize(), the clock, fn(step),
             torch.cuda.synchronize(), the clock.  Between the two synchronizes is only the call, so a value holds the host's
             work, the enqueue and the device's work to the last kernel, in milliseconds.  The result is dropped before the
             next way runs, the ways alternate inside every step, the first `warmup` steps are discarded, `steps` are kept.

stats() of the kept values is what the documents hold: median, p10 and p90, four places."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(v):
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}


def inside(parent_stats, stats):
    """The verdict `p10 <= median <= p90`: this tree's median lies inside the parent's spread"""
    return bool(parent_stats["p10"] <= stats["median"] <= parent_stats["p90"])


def not_above(parent_stats, stats):
    """The verdict `median <= p90`: inside the parent's spread or below it"""
    return bool(stats["median"] <= parent_stats["p90"])


def event_ms(torch, stream, ways, steps, warmup, reps, alternate, before=None):
    """{way: [ms per call, ...]} of ways {way: fn()}; `reps` one count, or {way: count} where the ways differ in it"""
    count = reps if isinstance(reps, dict) else dict.fromkeys(ways, reps)
    turns = range(steps + warmup)
    order = [(rep, way) for rep in turns for way in ways] if alternate else [(rep, way) for way in ways for rep in turns]
    kept = {way: [] for way in ways}
    for rep, way in order:
        fn, n = ways[way], count[way]
        if before is not None and way in before:
            before[way]()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        if rep >= warmup:
            kept[way].append(e0.elapsed_time(e1) / n)
    return kept


def wall_ms(torch, ways, steps, warmup, before=None):
    """{way: [ms, ...]} of ways {way: fn(step)}; before(step), if given, runs in front of every way's first synchronize"""
    synchronize, clock = torch.cuda.synchronize, time.perf_counter
    kept = {way: [] for way in ways}
    for i in range(steps + warmup):
        for way, fn in ways.items():
            if before is not None:
                before(i)
            synchronize()
            t0 = clock()
            out = fn(i)
            synchronize()
            t1 = clock()
            del out
            if i >= warmup:
                kept[way].append((t1 - t0) * 1e3)
    return kept


def load_parent(tree):
    """The package of another tree under another name (its own libalacgpu.so next to it)"""
    d = os.path.join(tree, "alac.net_amd")
    spec = importlib.util.spec_from_file_location("alac_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["alac_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def make_file(synth, frames, seed, rate=44100):
    """A synthetic M4A of `frames` frames: stereo 16-bit, 4096-frame packets, the last one short"""
    from alac.net_amd.synth import m4a

    n = -(-frames // 4096)
    d = synth.packet_descs(n, stereo=1)
    d["n"][-1] = frames - (n - 1) * 4096
    b = synth.make_batch(d, synth.default_signal(seed))
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    return m4a.write_m4a(packets, [int(x) for x in d["n"]], sample_size=16, channels=2, sample_rate=rate)


def arguments(ap, out, reps=None, parent=None):
    """--steps, --warmup, --reps (default `reps`, if the tool has it), --parent (help `parent`, if it has it) and --out"""
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    if reps is not None:
        ap.add_argument("--reps", type=int, default=reps)
    if parent is not None:
        ap.add_argument("--parent", help=parent)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))


def device(torch):
    """GPU 0 made current: (device, its current stream)"""
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    return dev, torch.cuda.current_stream(dev)


def command(tool):
    """The document's "command": the tool (its __file__) and the arguments it was given"""
    return f"python tools/{os.path.basename(tool)} " + " ".join(sys.argv[1:])


def emit(doc, out):
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    with open(out, "w") as f:
        f.write(text + "\n")
