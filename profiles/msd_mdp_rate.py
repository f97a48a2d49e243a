"""Cost of image flags and of the mean-squared displacement in the device integrator: ms per step of the resident C-ABI
path (mdp_md_integrate_check with the fused final half, as bench.py drives it) on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
in three modes on the same MI355X:
  (a) nve_parent  NVE with the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH)
  (b) nve         NVE with this build and no image: the remap, pack and permute kernels are the instantiations the parent
                  launches, so (b) must equal (a) within the box-to-box spread of the README (2-3 %)
  (c) msd         this build with image flags tracked (mdp_md_set_image: every reneighbouring reads and, for atoms that
                  left the box, rewrites 4 more bytes per atom, and permutes them) and a mean-squared displacement read
                  every 100 steps (two blocking calls: one pass over the atoms each).  No target: what it costs is recorded
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating; the fastest
run of each counts.  All modes reneighbor on the same steps: the alloy at a fixed interval (REBUILD_EVERY), REBO-MoS by
the on-device check (the builds of each mode are recorded).  The parent stops at the first child that does not end
cleanly.  Usage: python profiles/msd_mdp_rate.py [out.json] [--steps K] [--warmup W] [--parent-lib PATH]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = {"rebomos": (24, 24, 24), "aeam": (63, 63, 63)}
TEMPS = {"rebomos": 300.0, "aeam": 863.0}
REBUILD_EVERY = {"rebomos": 0, "aeam": 10}   # 0: the deferred on-device `check yes`
REPS = 2
SPREAD = 3.0   # per cent: (b) against (a)
MODES = ("nve_parent", "nve", "msd")


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
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)
    if mode == "msd":
        d.track_images()
        d.msd()
    d.compute(1, 0)
    thermo = 100
    every = REBUILD_EVERY[workload]

    msd = {}

    def run(n, k0):
        for k in range(1, n + 1):
            ev = 1 if (k0 + k) % thermo == 0 else 0
            rebuild = "auto" if not every else (k0 + k) % every == 0
            d.step(ev, 0, rebuild=rebuild, defer_final=not ev and k < n)
            if ev and mode == "msd":
                msd[k0 + k] = float(d.msd_read()[3])

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
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps, "ms_per_step": ms, "temp": t["temp"],
           "builds": d.builds - b0, "dangerous": d.dangerous, "msd": msd,
           "library": "the parent commit's (--parent-lib)" if os.environ.get("MDP_LIB_PATH") else "this build"}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 300
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 30
    parent = os.path.abspath(args[args.index("--parent-lib") + 1]) if "--parent-lib" in args else None
    out_path = next((a for a in args if a.endswith(".json")), None)
    modes = [m for m in MODES if m != "nve_parent" or parent]
    results = []
    runs = [(wl, mode) for wl in SYSTEMS for _ in range(REPS) for mode in modes]
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
    summary = {}
    for wl in SYSTEMS:
        best = {m: min((r for r in results if r["workload"] == wl and r["mode"] == m), key=lambda r: r["ms_per_step"])
                for m in modes}
        b, c = best["nve"], best["msd"]
        row = {"atoms": b["atoms"], "nve_ms": b["ms_per_step"], "msd_ms": c["ms_per_step"],
               "msd_extra_percent": 100.0 * (c["ms_per_step"] / b["ms_per_step"] - 1.0), "msd": c["msd"],
               "builds": {m: best[m]["builds"] for m in modes}}
        text = f"{wl}: {b['atoms']} atoms  NVE {b['ms_per_step']:.3f}"
        if parent:
            a = best["nve_parent"]
            row["nve_parent_ms"] = a["ms_per_step"]
            row["nve_against_parent_percent"] = 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0)
            row["spread_percent"] = SPREAD
            row["path_without_image_unchanged"] = row["nve_against_parent_percent"] <= SPREAD
            text += f" (parent {a['ms_per_step']:.3f}, {row['nve_against_parent_percent']:+.2f} %)"
        text += (f"  images + MSD every 100 steps {c['ms_per_step']:.3f} ({row['msd_extra_percent']:+.2f} %) ms/step; "
                 f"builds {row['builds']}; msd {c['msd']}")
        summary[wl] = row
        print(text)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"steps": steps, "warmup": warmup, "summary": summary, "results": results}, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
