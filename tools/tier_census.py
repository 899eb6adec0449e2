#!/usr/bin/env python3
"""Census of the entropy wave's tiers over the directed corpus of tests/tier_cases.py (runs ON THE GPU BOX, in the manner of
tools/stamps.py): every case through the diagnostic build and its unit counters (alac_diag.h).  A census, not a gate: no number
from it goes into any assertion.
usage: make -C alac.net_amd/csrc diag; ALACGPU_LIB=alac.net_amd/csrc/libalacgpu_diag.so python tools/tier_census.py"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import alac.net_amd as pkg
import tier_cases as tc

assert "_diag" in os.path.basename(os.environ.get("ALACGPU_LIB", "")), "set ALACGPU_LIB to the diagnostic build (make diag)"
COUNTERS = ["plain_ok", "fail_esc", "fail_run", "fail_range", "wide_units", "z_units", "esc_units", "full_units", "late_run", "redo"]
dev = torch.device("cuda", 0)
fn = pkg.lib().alacgpu_dbg_decode_batch_device_stamps
fn.restype = C.c_int
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def counters(b):
    n, slot, nb = len(b["sizes"]), int(b["slot_ints"]), int(b["blob"].size)
    d_blob = torch.zeros((nb + 63) // 16 * 16 + 64, dtype=torch.uint8, device=dev)
    d_blob[:nb] = torch.from_numpy(b["blob"]).to(dev)
    d_off = torch.from_numpy(b["offsets"].astype(np.int64)).to(dev)
    d_sz = torch.from_numpy(b["sizes"].astype(np.int32)).to(dev)
    d_ci = torch.from_numpy(b["cfg_idx"].astype(np.int16)).to(dev)
    d_pcm = torch.zeros((n, slot), dtype=torch.int32, device=dev)
    d_ob = torch.zeros(n, dtype=torch.int32, device=dev)
    d_os, d_st = torch.zeros_like(d_ob), torch.zeros_like(d_ob)
    d_stamps = torch.zeros(8 * ((n + 7) // 8), dtype=torch.int64, device=dev)
    with pkg.AlacGpuContext(b["stream_cfgs"]) as ctx:
        rc = fn(ctx._ctx, vp(d_blob), C.c_uint64(nb), vp(d_off), vp(d_sz), vp(d_ci), C.c_uint32(n), vp(d_pcm), C.c_uint32(slot),
                vp(d_ob), vp(d_os), vp(d_st), None, vp(d_stamps))
        assert rc == 0
        torch.cuda.synchronize()
    s = d_stamps.cpu().numpy().astype(np.uint64).reshape(-1, 8)
    hi = lambda x: int((x >> np.uint64(32)).sum())
    lo = lambda x: int((x & np.uint64(0xFFFFFFFF)).sum())
    f16 = lambda x, sh: int(((x >> np.uint64(sh)) & np.uint64(0xFFFF)).sum())
    return {"plain_ok": hi(s[:, 1]), "fail_esc": lo(s[:, 1]), "z_units": hi(s[:, 4]), "esc_units": lo(s[:, 4]),
            "fail_run": f16(s[:, 5], 48), "redo": f16(s[:, 5], 32), "full_units": f16(s[:, 6], 48), "late_run": f16(s[:, 6], 32),
            "wide_units": hi(s[:, 7]), "fail_range": lo(s[:, 7])}


print("unit counters of the diagnostic build (units of 16, narrow step off), summed over both passes and the workgroups of a case;")
print("per case: mono 16-bit and stereo 24-bit, LPC orders 1..8")
print(f"{'case':<18s}" + "".join(f"{c:>11s}" for c in COUNTERS))
total = dict.fromkeys(COUNTERS, 0)
rows = [(name, tc.build(name, st, i24, "first_launch")) for name in tc.CASES for st, i24 in ((False, False), (True, True))]
rows += [(f"fir_{kind}", tc.build_fir(kind, st, i24, 0)) for kind in tc.FIR_KINDS for st, i24 in ((False, False), (True, True))]
for name, g in rows:
    c = counters(g.batch())
    nc = g.cfgs[0][5]
    print(f"{name + ('/s24' if nc == 2 else '/m16'):<18s}" + "".join(f"{c[k]:>11d}" for k in COUNTERS), flush=True)
    for k in COUNTERS:
        total[k] += c[k]
print(f"{'corpus':<18s}" + "".join(f"{total[k]:>11d}" for k in COUNTERS))
zero = [k for k in COUNTERS if total[k] == 0]
print("counters that stayed zero over the corpus: " + (", ".join(zero) if zero else "none"))
