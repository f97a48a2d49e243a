"""What the prescribed group forces cost in resident mode, and that a run without them is undisturbed: ms per step of the
resident C-ABI path (mdp_md_integrate_check with the deferred final half, as bench.py drives it) on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
in four modes on the same MI355X:
  (a) nve_parent  NVE with the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH)
  (b) nve         NVE with this build and no group forces: accepted when (b) - (a) lies inside the spread of (a)'s own
                  repetitions in this session (both spreads are recorded)
  (c) set         this build with one setforce 0 0 0 grip on a sixth of the box (the slab x < 1/6, a group bit: the mask is
                  read): no aveforce is on, so gforce_sums_kernel writes f itself and gforce_control_kernel follows
  (d) setave      setforce 0 0 NULL and aveforce NULL NULL -0.001 on that one group: gforce_sums_kernel,
                  gforce_control_kernel and gforce_apply_kernel in front of every step's fused kick
The gripped slab starts at rest, so it stays where it is and the lists of all modes see the same motion elsewhere.
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating and their order
rotating from one repetition to the next; the fastest run of each counts and every run is kept in the JSON.  All modes
reneighbor by the same rule: the alloy at a fixed interval (REBUILD_EVERY), REBO-MoS by the on-device check.  The parent
stops at the first child that does not end cleanly.
--kernels DIR: the per-kernel times of modes (c) and (d) from `rocprofv3 --kernel-trace` runs of their own (one child per
system and mode, profiler on, its ms per step not used), medians over the run, written into the JSON.
Usage: python profiles/gforce_mdp_rate.py [out.json] [--steps K] [--warmup W] [--reps R] [--parent-lib PATH] [--kernels DIR]"""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = {"rebomos": (24, 24, 24), "aeam": (63, 63, 63)}
TEMPS = {"rebomos": 300.0, "aeam": 863.0}
REBUILD_EVERY = {"rebomos": 0, "aeam": 10}   # 0: the deferred on-device `check yes`
REPS = 3
MODES = ("nve_parent", "nve", "set", "setave")
STAGE = ("set", "setave")
KERNELS = ("gforce_sums_kernel", "gforce_control_kernel", "gforce_apply_kernel", "nve_advance_kernel")
GRIP_BIT = 2


def child(workload, mode, steps, warmup):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.load_package()
    import numpy as np
    import torch
    from lammps_plugins_amd.host import capi, resident, system as S
    gold = os.path.join(ROOT, "tests", "golden", "potentials")
    rep = SYSTEMS[workload]
    ctx = capi.Context(0)
    if workload == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), rep)
        p = capi.read_rebomos_file(os.path.join(gold, "MoS.REBO.set5b"))
        ctx.rebomos_set_params(p)
        style, skin, map_, cutghost = capi.STYLE_REBOMOS, 2.0, [0, 0, 1], 3.0 * p.rcmax[0][0] + 2.0
    else:
        af = capi.AeamFile(os.path.join(gold, "AlSi.aeam"))
        s = S.fcc_cell(4.045, rep, frac_type2=0.0075, seed=7683797)
        s.mass[1:3] = af.mass[:2]
        tabs = af.build()
        ctx.aeam_set_tables(tabs)
        style, skin, map_, cutghost = capi.STYLE_AEAM, 1.0, None, float(af.cut_table(tabs).max()) + 1.0
    v0 = S.gaussian_velocities(s, 2.0 * TEMPS[workload], seed=1082337)   # (equipartition gives half of it to the lattice)
    grip = s.box.x2lamda(S.wrap(s.box, s.x))[:, 0] < 1.0 / 6.0
    if mode in STAGE:
        v0 = v0.copy()
        v0[grip] = 0.0
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps,
           "library": "the parent commit's (--parent-lib)" if os.environ.get("MDP_LIB_PATH") else "this build"}
    d.compute(1, 0)
    if mode in STAGE:          # (behind the setup compute, as fix nve/mdp's setup() does it)
        by_tag = np.ones(s.n + 1, dtype=np.int32)
        by_tag[s.tag[grip]] |= GRIP_BIT
        d.set_group(by_tag, 0)
        if mode == "set":
            d.gforce([dict(kind="set", f=(0.0, 0.0, 0.0), bit=GRIP_BIT)])
        else:
            d.gforce([dict(kind="set", f=(0.0, 0.0, None), bit=GRIP_BIT), dict(kind="ave", f=(None, None, -0.001), bit=GRIP_BIT)])
    thermo = 100
    every = REBUILD_EVERY[workload]

    def run(n, k0):
        for k in range(1, n + 1):
            ev = 1 if (k0 + k) % thermo == 0 else 0
            rebuild = "auto" if not every else (k0 + k) % every == 0
            d.step(ev, 0, rebuild=rebuild, defer_final=not ev and k < n)

    run(warmup, 0)
    d.flush()
    b0 = d.builds
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    run(steps, warmup)
    d.flush()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    t = d.thermo()
    out.update({"ms_per_step": ms, "temp": t["temp"], "builds": d.builds - b0, "dangerous": d.dangerous})
    if mode in STAGE:
        st = d.gforce_state(0)
        assert st["passes"] == steps + warmup + 1 and st["step"] == steps + warmup and st["atoms"] == int(grip.sum()), st
        out["grip_atoms"], out["fx"] = st["atoms"], float(st["ftotal"][0])
    print("RESULT " + json.dumps(out), flush=True)


def kernel_medians(path):
    """{kernel: (median us, launches)} of the kernels of KERNELS from the kernel trace under path"""
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    times = {}
    for r in rows:
        name = re.sub(r"\(.*$", "", r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", ""))
        name = re.sub(r"<.*$", "", name)
        if name in KERNELS:
            times.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (sorted(v)[len(v) // 2], len(v)) for k, v in times.items()}


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 300
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 30
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else REPS
    parent = os.path.abspath(args[args.index("--parent-lib") + 1]) if "--parent-lib" in args else None
    kdir = os.path.abspath(args[args.index("--kernels") + 1]) if "--kernels" in args else None
    only = args[args.index("--systems") + 1].split(",") if "--systems" in args else list(SYSTEMS)
    out_path = next((a for a in args if a.endswith(".json")), None)
    modes = [m for m in MODES if m != "nve_parent" or parent]
    results = []
    runs = [(wl, mode) for wl in only for rep in range(reps) for mode in modes[rep % len(modes):] + modes[:rep % len(modes)]]
    for wl, mode in runs:
        cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", wl,
               "nve" if mode == "nve_parent" else mode, str(steps), str(warmup)]
        env = dict(os.environ)
        env.pop("MDP_LIB_PATH", None)
        if mode == "nve_parent":
            env["MDP_LIB_PATH"] = parent
        p = subprocess.run(cmd, capture_output=True, text=True, env=env)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            print(f"{wl} {mode}: exit status {p.returncode}; stopping", file=sys.stderr)
            sys.exit(1)
        r = json.loads(lines[-1][7:])
        r["mode"] = mode
        results.append(r)
        print(json.dumps(r), flush=True)
    kernels = {}
    if kdir:   # the profiler in runs of its own: kernel times only
        for wl in only:
            kernels[wl] = {}
            for mode in STAGE:
                path = os.path.join(kdir, wl + "-" + mode)
                cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", path, "--",
                       sys.executable, os.path.abspath(__file__), "--child", wl, mode, "60", "10"]
                env = dict(os.environ)
                env.pop("MDP_LIB_PATH", None)
                p = subprocess.run(cmd, capture_output=True, text=True, env=env)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                    print(f"{wl} {mode} kernel trace: exit status {p.returncode}; stopping", file=sys.stderr)
                    sys.exit(1)
                kernels[wl][mode] = {k: {"median_us": v[0], "launches": v[1]} for k, v in kernel_medians(path).items()}
                print(json.dumps({wl: {mode: kernels[wl][mode]}}), flush=True)
    summary = {}
    for wl in only:
        of = lambda m: [r for r in results if r["workload"] == wl and r["mode"] == m]
        best = {m: min(of(m), key=lambda r: r["ms_per_step"]) for m in modes}
        spread = lambda m: 100.0 * (max(r["ms_per_step"] for r in of(m)) / best[m]["ms_per_step"] - 1.0)
        b = best["nve"]
        row = {"atoms": b["atoms"], "nve_ms": b["ms_per_step"], "nve_spread_percent": spread("nve"),
               "all_runs_ms": {m: sorted(round(r["ms_per_step"], 4) for r in of(m)) for m in modes},
               "builds": {m: best[m]["builds"] for m in modes}}
        text = f"{wl}: {b['atoms']} atoms  NVE {b['ms_per_step']:.3f} (spread {row['nve_spread_percent']:.2f} %)"
        if parent:
            a = best["nve_parent"]
            row["nve_parent_ms"], row["nve_parent_spread_percent"] = a["ms_per_step"], spread("nve_parent")
            row["nve_against_parent_percent"] = 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0)
            row["run_undisturbed"] = row["nve_against_parent_percent"] <= max(row["nve_parent_spread_percent"], 0.5)
            text += f"  parent {a['ms_per_step']:.3f} (spread {row['nve_parent_spread_percent']:.2f} %), {row['nve_against_parent_percent']:+.2f} %"
        for m in STAGE:
            c = best[m]
            row[m] = {"ms": c["ms_per_step"], "spread_percent": spread(m), "extra_ms": c["ms_per_step"] - b["ms_per_step"],
                      "extra_percent": 100.0 * (c["ms_per_step"] / b["ms_per_step"] - 1.0), "grip_atoms": c["grip_atoms"]}
            text += f"  {m} {c['ms_per_step']:.3f} ms/step ({row[m]['extra_ms']:+.3f} ms, {row[m]['extra_percent']:+.1f} %, spread {row[m]['spread_percent']:.2f} %)"
            if wl in kernels and m in kernels[wl]:
                row[m]["kernels"] = kernels[wl][m]
                row[m]["new_kernels_us"] = sum(v["median_us"] for k, v in kernels[wl][m].items() if k != "nve_advance_kernel")
                text += " [" + ", ".join(f"{k} {v['median_us']:.1f} us" for k, v in kernels[wl][m].items()) + "]"
        text += f"; builds {row['builds']}"
        summary[wl] = row
        print(text)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"steps": steps, "warmup": warmup, "reps": reps, "summary": summary, "results": results}, f, indent=1)
    if parent and not all(row["run_undisturbed"] for row in summary.values()):
        print("NVE with this build is outside the spread of the parent library's own repetitions: a finding", file=sys.stderr)
        sys.exit(2)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
