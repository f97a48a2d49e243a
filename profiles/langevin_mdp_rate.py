"""Cost of the device Langevin thermostat: ms per step of the resident C-ABI path (mdp_md_integrate_check with the fused
final half, as bench.py drives it) in NVE against Langevin (mdp_langevin_*, damp 0.1 ps) and against Langevin with
`zero yes tally yes`, on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating; the fastest
run of each counts.  All modes reneighbor on the same steps: the alloy at a fixed interval (REBUILD_EVERY; its
displacement-triggered rebuilds would differ between the two trajectories and mix list builds into the difference),
REBO-MoS by the on-device check (the builds of each mode are recorded).  The parent stops at the first child that does
not end cleanly.  Usage: python profiles/langevin_mdp_rate.py [out.json] [--steps K] [--warmup W]"""
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
GOAL = 1.0   # per cent: Langevin (no zero / tally) step time over NVE step time
LIMIT = 5.0  # per cent: beyond it the cost is a defect
MODES = ("nve", "langevin", "langevin_zero_tally")


def child(workload, mode, steps, warmup):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.load_package()
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
    # NVE starts at twice the temperature: equipartition gives half of it to the lattice, so that every mode runs at about
    # the same temperature (the thermostat holds TEMPS from TEMPS) and the modes differ in the integrate kernel alone
    v0 = S.gaussian_velocities(s, (2.0 if mode == "nve" else 1.0) * TEMPS[workload], seed=1082337)
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)
    if mode != "nve":
        zt = mode == "langevin_zero_tally"
        d.langevin(TEMPS[workload], TEMPS[workload], 0.1, 48271, zero=zt, tally=zt, first=0, last=warmup + steps)
    d.compute(1, 0)
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
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps, "ms_per_step": ms, "temp": t["temp"],
           "builds": d.builds - b0, "dangerous": d.dangerous}
    if mode != "nve":
        out["ecouple"] = d.langevin_tally()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 500
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 50
    out_path = next((a for a in args if a.endswith(".json")), None)
    results = []
    runs = [(wl, mode) for wl in SYSTEMS for _ in range(REPS) for mode in MODES]
    for wl, mode in runs:
        cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", wl, mode, str(steps),
               str(warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            print(f"{wl} {mode}: exit status {p.returncode}; stopping", file=sys.stderr)
            sys.exit(1)
        r = json.loads(lines[-1][7:])
        results.append(r)
        print(json.dumps(r), flush=True)
    summary = {}
    for wl in SYSTEMS:
        a = min((r for r in results if r["workload"] == wl and r["mode"] == "nve"), key=lambda r: r["ms_per_step"])
        b = min((r for r in results if r["workload"] == wl and r["mode"] == "langevin"), key=lambda r: r["ms_per_step"])
        z = min((r for r in results if r["workload"] == wl and r["mode"] == "langevin_zero_tally"),
                key=lambda r: r["ms_per_step"])
        extra = 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0)
        extra_zt = 100.0 * (z["ms_per_step"] / a["ms_per_step"] - 1.0)
        summary[wl] = {"atoms": a["atoms"], "nve_ms": a["ms_per_step"], "langevin_ms": b["ms_per_step"],
                       "langevin_zero_tally_ms": z["ms_per_step"], "extra_percent": extra,
                       "extra_zero_tally_percent": extra_zt, "builds": [a["builds"], b["builds"], z["builds"]],
                       "goal_percent": GOAL, "limit_percent": LIMIT, "within_limit": extra <= LIMIT}
        print(f"{wl}: {a['atoms']} atoms  NVE {a['ms_per_step']:.3f}  Langevin {b['ms_per_step']:.3f} (+{extra:.2f} %)  "
              f"zero+tally {z['ms_per_step']:.3f} (+{extra_zt:.2f} %) ms/step; builds {a['builds']} / {b['builds']} / "
              f"{z['builds']}")
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"steps": steps, "warmup": warmup, "summary": summary, "results": results}, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
