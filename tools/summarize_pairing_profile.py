"""profiles/pairing_dense_pmc_summary_cfg2.json, profiles/traffic_cfg2.json and the two kernel-stats tables (profiles/pairing_dense_kernel_stats_cfg2*.csv) from a directory of rocprofv3 runs of
bench.py --config 2 --steps 12 --warmup 3 (one --kernel-trace --stats run of the parent tree in stats_parent/, of this tree in stats_cfg2/, and one
--pmc run per counter group in pmc_fetch_cfg2/, pmc_write_cfg2/, pmc_sq_cfg2/).  Figures are medians over calls 4..15: the first call finds
nothing remembered.   usage (repository root): python tools/summarize_pairing_profile.py DIR"""
import csv, glob, json, collections, sys, shutil
import os
sys.path.insert(0, os.getcwd())
import bench
P = sys.argv[1]
def trace(d):
    rows = [r for r in csv.DictReader(open(glob.glob(f"{P}/{d}/*/*_kernel_trace.csv")[0])) if "alac" in r["Kernel_Name"]]
    per = collections.defaultdict(list)
    for r in rows: per[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return per
def warm(v): return v[3:]      # the first call is cold (nothing remembered), the next two settle: as bench.py's --warmup 3
def pmc(d):
    per = collections.defaultdict(lambda: collections.defaultdict(dict))
    for r in csv.DictReader(open(glob.glob(f"{P}/{d}/*/*_counter_collection.csv")[0])):
        if "alac" in r["Kernel_Name"]:
            per[r["Kernel_Name"]][r["Counter_Name"]][int(r["Dispatch_Id"])] = per[r["Kernel_Name"]][r["Counter_Name"]].get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    return {k: {c: [v[i] for i in sorted(v)] for c, v in d2.items()} for k, d2 in per.items()}
med = lambda v: sorted(v)[len(v) // 2]
doc = {"command": "rocprofv3 --kernel-trace --stats / --kernel-trace --pmc <one counter group per run> --output-format csv -- python3 bench.py --config 2 --steps 12 "
                  "--warmup 3 --no-cpu-baseline --no-host-path --no-big-batch --no-in-flight (15 calls; the figures are over calls 4..15: call 1 finds nothing remembered)",
       "workload": "cfg2, 4096 packets, 2 x 4096 x 4096 samples per call"}
for tag, d in (("parent", "stats_parent"), ("this_tree", "stats_cfg2")):
    t = trace(d)
    doc[f"kernel_ns_{tag}"] = {k: {"median": med(warm(v)), "min": min(warm(v)), "max": max(warm(v)), "first_call": v[0]} for k, v in t.items()}
    doc[f"launch_ns_{tag}"] = sum(med(warm(v)) for v in t.values())
fe, wr, sq = pmc("pmc_fetch_cfg2"), pmc("pmc_write_cfg2"), pmc("pmc_sq_cfg2")
samples = 2 * 4096 * 4096
tot = lambda p, c: sum(med(warm(v[c])) for v in p.values() if c in v)
fetch_kb, write_kb, valu = tot(fe, "FETCH_SIZE"), tot(wr, "WRITE_SIZE"), tot(sq, "SQ_INSTS_VALU")
doc["per_kernel"] = {k: {"FETCH_SIZE_KB": med(warm(fe[k]["FETCH_SIZE"])), "WRITE_SIZE_KB": med(warm(wr[k]["WRITE_SIZE"])),
                         "SQ_INSTS_VALU": med(warm(sq[k]["SQ_INSTS_VALU"])), "SQ_INSTS_SALU": med(warm(sq[k]["SQ_INSTS_SALU"])), "SQ_INSTS_LDS": med(warm(sq[k]["SQ_INSTS_LDS"])),
                         "first_call": {"FETCH_SIZE_KB": fe[k]["FETCH_SIZE"][0], "WRITE_SIZE_KB": wr[k]["WRITE_SIZE"][0], "SQ_INSTS_VALU": sq[k]["SQ_INSTS_VALU"][0]}} for k in fe}
gui = tot(wr, "GRBM_GUI_ACTIVE"); 
main = "alac_decode_ab_pair_dense_kernel"
wt = collections.defaultdict(list)
doc["traffic"] = {"FETCH_SIZE_KB_raw": fetch_kb, "WRITE_SIZE_KB": write_kb, "read_bytes_per_launch": 2 * fetch_kb * 1024, "write_bytes_per_launch": write_kb * 1024,
                  "hbm_bytes_per_launch": 2 * fetch_kb * 1024 + write_kb * 1024, "bytes_per_sample": (2 * fetch_kb * 1024 + write_kb * 1024) / samples,
                  "gfx950_correction": "read bytes = 2 x FETCH_SIZE x 1024 (as profiles/r3_final_pmc_summary_cfg2.json); WRITE_SIZE is exact"}
doc["issue"] = {"valu_wave_instr_per_launch": valu, "valu_wave_instr_per_sample": valu / samples}
old = json.load(open("profiles/r3_final_pmc_summary_cfg2.json"))
doc["two_pass_before"] = {"hbm_bytes_per_launch": old["traffic"]["hbm_bytes_per_launch"], "valu_wave_instr_per_sample": old["issue"].get("valu_wave_instr_per_sample"), "source": "profiles/r3_final_pmc_summary_cfg2.json"}
json.dump(doc, open("profiles/pairing_dense_pmc_summary_cfg2.json", "w"), indent=1)
oldt = json.load(open("profiles/traffic_cfg2.json"))
json.dump({"workload": "cfg2", "kernel": main, "hbm_bytes_per_launch": doc["traffic"]["hbm_bytes_per_launch"], "valu_wave_instr_per_launch": valu,
           "effective_clock_GHz": oldt["effective_clock_GHz"], "kernel_source_sha": bench.kernel_source_sha(), "source": "profiles/pairing_dense_pmc_summary_cfg2.json"},
          open("profiles/traffic_cfg2.json", "w"))
shutil.copy(glob.glob(f"{P}/stats_cfg2/*/*_kernel_stats.csv")[0], "profiles/pairing_dense_kernel_stats_cfg2.csv")
shutil.copy(glob.glob(f"{P}/stats_parent/*/*_kernel_stats.csv")[0], "profiles/pairing_dense_kernel_stats_cfg2_parent.csv")
print(json.dumps({k: doc[k] for k in ("kernel_ns_parent", "kernel_ns_this_tree", "launch_ns_parent", "launch_ns_this_tree", "traffic", "issue", "two_pass_before", "per_kernel")}, indent=1))
