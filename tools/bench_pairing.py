"""The paired decode against the parent commit's library, both packages in one process on one GPU (--parent DIR, a built tree of
the parent commit): decode_batch_device per call (tools/_measure.py: event_ms, the ways taking turns inside every repetition) --
  parent   the parent's package, the same resident packets every call
  warm     this tree, the same resident packets every call (what bench.py's steps are): the paired kernel decodes them
  off      this tree with set_pairing(False): the two-pass kernels alone
  cold     this tree, pairing on, the packets at an address it has not seen in every call (a copy of the blob per repetition):
           the paired kernel finds nothing, and after a window of such calls the context stops launching it
  rot8     this tree, a working set of 8 copies of the batch taking turns: inside the table's capacity (64 entries per packet)
  rot32    the same with 32 copies: more packets than the table has entries, every call finds its entries evicted
for cfg2 at 4096, 2048 and 1024 packets; cfg4 at 4096 packets (one-channel packets: nothing to pair), cfg3 and cfg5 at 4096 (orders
above 8: the paired kernel leaves every group) and cfg2 at 32768 packets (a batch above 4096: no paired launch) as parent / warm
only.  A gain counts when this tree's p90 lies more than 3 % below the parent's p10.
  python tools/bench_pairing.py --parent DIR [--out profiles/pairing_cfg2.json]"""
import argparse

from _measure import arguments, command, device, emit, event_ms, load_parent, stats


def resident(torch, dev, b):
    nb = int(b["blob"].size)
    blob = torch.zeros((nb + 63) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    blob[:nb] = torch.from_numpy(b["blob"].copy()).to(dev)
    n = len(b["sizes"])
    t = dict(blob=blob, nb=nb, n=n, slot=int(b["slot_ints"]),
             off=torch.from_numpy(b["offsets"].astype("int64")).to(dev), sz=torch.from_numpy(b["sizes"].astype("int32")).to(dev),
             pcm=torch.empty((n, int(b["slot_ints"])), dtype=torch.int32, device=dev))
    for k in ("ob", "os", "st"):
        t[k] = torch.empty(n, dtype=torch.int32, device=dev)
    return t


def call(ctx, t, stream, blob=None):
    ctx.decode_batch_device(t["blob"] if blob is None else blob, t["nb"], t["off"], t["sz"], t.get("ci"), t["n"], t["pcm"], t["slot"], t["ob"],
                            t["os"], t["st"], stream=stream.cuda_stream)


def main():
    ap = argparse.ArgumentParser()
    arguments(ap, "pairing_cfg2.json", parent="a built tree of the parent commit")
    a = ap.parse_args()
    import torch

    import alac.net_amd as pkg
    from alac.net_amd import synth

    parent = load_parent(a.parent)
    dev, stream = device(torch)
    doc = {"command": command(__file__).replace(a.parent, "DIR").replace(" --out " + a.out, ""), "steps": a.steps, "warmup": a.warmup, "unit": "ms per call (HIP events)", "cases": {}}
    for cfg, n, full in ((2, 4096, True), (2, 2048, True), (2, 1024, True), (4, 4096, False), (3, 4096, False), (5, 4096, False),
                         (2, 32768, False)):
        b = synth.make_config_batch(cfg, n_packets=n)
        t = resident(torch, dev, b)
        if b["cfg_idx"] is not None:
            t["ci"] = torch.from_numpy(b["cfg_idx"].astype("int16")).to(dev)
        with parent.AlacGpuContext(b["stream_cfgs"]) as pc, pkg.AlacGpuContext(b["stream_cfgs"]) as wc, \
                pkg.AlacGpuContext(b["stream_cfgs"]) as oc, pkg.AlacGpuContext(b["stream_cfgs"]) as cc, \
                pkg.AlacGpuContext(b["stream_cfgs"]) as r8, pkg.AlacGpuContext(b["stream_cfgs"]) as r32:
            oc.set_pairing(False)
            ways = {"parent": lambda: call(pc, t, stream), "warm": lambda: call(wc, t, stream)}
            before = None
            if full:
                copies = [t["blob"].clone() for _ in range(a.steps + a.warmup)]
                turn = iter(copies)
                fresh = {}
                rot = {"rot8": 0, "rot32": 0}
                before = {"cold": lambda: fresh.__setitem__("blob", next(turn)),
                          "rot8": lambda: rot.__setitem__("rot8", (rot["rot8"] + 1) % 8),
                          "rot32": lambda: rot.__setitem__("rot32", (rot["rot32"] + 1) % 32)}
                ways.update(off=lambda: call(oc, t, stream), cold=lambda: call(cc, t, stream, fresh["blob"]),
                            rot8=lambda: call(r8, t, stream, copies[rot["rot8"]]), rot32=lambda: call(r32, t, stream, copies[rot["rot32"]]))
            kept = event_ms(torch, stream, ways, a.steps, a.warmup, 1, True, before)
            case = {way: stats(v) for way, v in kept.items()}
            case["warm_p90_over_parent_p10"] = round(case["warm"]["p90"] / case["parent"]["p10"], 4)
            case["pairing_stats_warm"] = list(wc.pairing_stats())
            if full:
                case["pairing_stats_cold"] = list(cc.pairing_stats())
                case["pairing_stats_rot8"] = list(r8.pairing_stats())
                case["pairing_stats_rot32"] = list(r32.pairing_stats())
            doc["cases"][f"cfg{cfg}_{n}"] = case
            del t, b
            torch.cuda.empty_cache()
    emit(doc, a.out)


if __name__ == "__main__":
    main()
