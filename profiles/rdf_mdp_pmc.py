"""What binds the histogram kernel of compute rdf/mdp: rocprofv3 passes over `profiles/rdf_mdp_rate.py --child WORKLOAD reads N 0`
(setup, one compute, N blocking reads of 200 bins x 3 columns at the cutoff limit), each pass a process of its own under
`timeout -k 10`:
  stats   --kernel-trace --stats: device time of the kernels of a read (no counters in this pass)
  sq1     --pmc, counters only: waves, wave-cycles, busy cycles, waits, VALU activity and instruction count
  sq2     --pmc, counters only: vector-memory, scalar and LDS instruction counts, LDS activity, bank conflicts, LDS waits
Counters and tracing are never combined.  The rows of the rdf_* kernels (and of the sort between them) are averaged over
the N reads and written, with the launch geometry rocprofv3 reports, to the JSON; the stored figures are what DESIGN.md
section 4 quotes.  The passes stop at the first one that does not end cleanly.
Usage: python profiles/rdf_mdp_pmc.py out.json [--workload rebomos|aeam] [--reads N]"""
import collections
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = [
    ("stats", ["--kernel-trace", "--stats"]),
    ("sq1", ["--pmc", "SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY",
             "SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU"]),
    ("sq2", ["--pmc", "SQ_INSTS_VMEM_RD", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VMEM", "SQ_ACTIVE_INST_LDS",
             "SQ_LDS_BANK_CONFLICT", "SQ_INST_CYCLES_VMEM", "SQ_WAIT_INST_LDS"]),
]


def short(name):
    for k in ("rdf_hist_kernel", "rdf_assign_kernel", "rdf_bounds_kernel", "rdf_tail_kernel"):
        if k in name:
            return k
    return None


def main():
    args = sys.argv[1:]
    out_path = next(a for a in args if a.endswith(".json"))
    workload = args[args.index("--workload") + 1] if "--workload" in args else "rebomos"
    reads = int(args[args.index("--reads") + 1]) if "--reads" in args else 3
    child = [sys.executable, os.path.join(ROOT, "profiles", "rdf_mdp_rate.py"), "--child", workload, "reads", str(reads), "0"]
    out = {"workload": workload, "reads": reads, "command": "rocprofv3 <pass> --output-format csv -d DIR -- python profiles/rdf_mdp_rate.py --child "
           f"{workload} reads {reads} 0", "passes": {name: " ".join(opts) for name, opts in PASSES}}
    for name, opts in PASSES:
        d = tempfile.mkdtemp(prefix="rdf_pmc_")
        try:
            p = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", *opts, "--output-format", "csv", "-d", d, "--", *child],
                               capture_output=True, text=True)
            result = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not result:
                print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                print(f"pass {name}: exit status {p.returncode}; stopping", file=sys.stderr)
                sys.exit(1)
            out.setdefault("run", json.loads(result[-1][7:]))
            if name == "stats":
                rows = {}
                for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    for r in csv.DictReader(open(f)):
                        k = short(r["Name"])
                        if k:
                            rows[k] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                                       "max_ns": float(r["MaxNs"])}
                        elif "radix_sort" in r["Name"] and "unsigned int, int" in r["Name"]:   # the read's sort: 32-bit cell keys
                            e = rows.setdefault("rocprim radix sort, unsigned int keys (all its kernels; list builds use it too)",
                                                {"calls": 0, "total_ns": 0.0})
                            e["calls"] += int(r["Calls"])
                            e["total_ns"] += float(r["TotalDurationNs"])
                out["kernel_time"] = rows
            else:
                acc, geom = collections.defaultdict(lambda: collections.defaultdict(list)), {}
                for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                    for r in csv.DictReader(open(f)):
                        k = short(r["Kernel_Name"])
                        if k:
                            acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
                            geom[k] = {"grid_size": int(r["Grid_Size"]), "workgroup_size": int(r["Workgroup_Size"]),
                                       "lds_block_size": int(r["LDS_Block_Size"]), "vgpr_count": int(r["VGPR_Count"]),
                                       "sgpr_count": int(r["SGPR_Count"]), "scratch_size": int(r["Scratch_Size"])}
                for k, counters in acc.items():
                    e = out.setdefault("counters", {}).setdefault(k, {"launch": geom[k], "mean_per_dispatch": {}, "dispatches": 0})
                    for cname, vals in counters.items():
                        e["mean_per_dispatch"][cname] = sum(vals) / len(vals)
                        e["dispatches"] = len(vals)
            print(f"pass {name} done", flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    h = out.get("counters", {}).get("rdf_hist_kernel", {}).get("mean_per_dispatch", {})
    if h.get("SQ_WAVE_CYCLES") and h.get("SQ_WAVES"):
        waves_per_simd = 8.0   # the launch: 8 workgroups of 4 waves per CU when the histogram is small (rdf.hip)
        out["derived"] = {
            "valu_busy_fraction_of_a_simd": h["SQ_ACTIVE_INST_VALU"] / (h["SQ_WAVE_CYCLES"] / waves_per_simd),
            "assumed_waves_per_simd": waves_per_simd,
            "wait_fraction_of_wave_cycles": h["SQ_WAIT_ANY"] / h["SQ_WAVE_CYCLES"],
            "valu_instructions_per_record_load": h["SQ_INSTS_VALU"] / h["SQ_INSTS_VMEM_RD"] if h.get("SQ_INSTS_VMEM_RD") else None,
            "lds_instructions_per_valu_instruction": h["SQ_INSTS_LDS"] / h["SQ_INSTS_VALU"] if h.get("SQ_INSTS_LDS") else None,
            "lds_bank_conflict_fraction_of_wave_cycles": h["SQ_LDS_BANK_CONFLICT"] / h["SQ_WAVE_CYCLES"] if h.get("SQ_LDS_BANK_CONFLICT") else None,
            "lane_slots_of_record_loads": 64.0 * h["SQ_INSTS_VMEM_RD"] if h.get("SQ_INSTS_VMEM_RD") else None,
        }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out.get("derived", {})))


if __name__ == "__main__":
    main()
