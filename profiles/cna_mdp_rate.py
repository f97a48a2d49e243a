"""What `compute cna/atom/mdp` costs, and that the run itself is undisturbed: the resident C-ABI path (mdp_md_integrate_check with
the fused final half, as bench.py drives it) on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
in three modes on the same MI355X:
  (a) nve_parent  ms per NVE step with the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH)
  (b) nve         ms per NVE step with this build and no measurement: no step code changed, so (b) is expected inside the
                  repetitions' spread of (a); both figures and the spreads are reported, nothing is asserted
  (c) reads       this build, after the warm-up steps: blocking reads on their own, timed with a host clock around calls
                  that end in a device synchronise, READS of each after one untimed read (the buffers of the binning
                  exist before the timed window).  A per-atom read includes the device-to-host copy of its values (8 bytes
                  per atom) and of the owned atoms' tags (4 bytes per atom).
                    cna    cna/atom/mdp at Rc = 2.8 A (MoS2: every centre leaves at n not in {12, 14}) / 3.45 A (the alloy:
                           12 neighbours, every centre takes the whole path); next to it the read of coord/atom/mdp at the
                           same cutoff with one column over all types, which bins the same atoms and walks the same stencil
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating and their order
rotating from one repetition to the next; the fastest run of each counts, and every run and the spread (max / min - 1) of
each are kept in the JSON.  The parent stops at the first child that does not end cleanly.
Usage: python profiles/cna_mdp_rate.py [out.json] [--steps K] [--warmup W] [--parent-lib PATH]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = {"rebomos": (24, 24, 24), "aeam": (63, 63, 63)}
TEMPS = {"rebomos": 300.0, "aeam": 863.0}
REBUILD_EVERY = {"rebomos": 0, "aeam": 10}   # 0: the deferred on-device `check yes`
REPS = 3
READS = 5
MODES = ("nve_parent", "nve", "reads")
CNA_RC = {"rebomos": 2.8, "aeam": 3.45}


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
    d.compute(1, 0)
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps,
           "library": "the parent commit's (--parent-lib)" if os.environ.get("MDP_LIB_PATH") else "this build"}
    every = REBUILD_EVERY[workload]

    def run(n, k0):
        for k in range(1, n + 1):
            ev = 1 if (k0 + k) % 100 == 0 else 0
            rebuild = "auto" if not every else (k0 + k) % every == 0
            d.step(ev, 0, rebuild=rebuild, defer_final=not ev and k < n)

    run(warmup, 0)
    d.flush()
    if mode == "reads":
        def timed(read):
            read()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(READS):
                got = read()
            return (time.perf_counter() - t0) * 1e3 / READS, got

        rc = CNA_RC[workload]
        d.coord(rc)
        coord_ms, got = timed(d.coord_read)
        partners = int(got[1].sum())
        d.cna(rc)
        cna_ms, got = timed(d.cna_read)
        out["cases"] = {"cna": {"cutoff": rc, "read_ms": cna_ms, "coord_read_ms": coord_ms, "partners_in_coord": partners,
                                "census": [int(v) for v in ctx.cna_counts()], "over": ctx.cna_info()["over"],
                                "census_is_the_histogram": bool(np.array_equal(np.bincount(got[1].astype(np.int64), minlength=6), ctx.cna_counts())),
                                "bytes_to_host": int(got[1].nbytes + got[0].nbytes)}}
        print("RESULT " + json.dumps(out), flush=True)
        return
    b0 = d.builds
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    run(steps, warmup)
    d.flush()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out.update({"ms_per_step": ms, "temp": d.thermo()["temp"], "builds": d.builds - b0, "dangerous": d.dangerous})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 300
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 30
    parent = os.path.abspath(args[args.index("--parent-lib") + 1]) if "--parent-lib" in args else None
    out_path = next((a for a in args if a.endswith(".json")), None)
    modes = [m for m in MODES if m != "nve_parent" or parent]
    results = []
    runs = [(wl, mode) for wl in SYSTEMS for rep in range(REPS) for mode in modes[rep % len(modes):] + modes[:rep % len(modes)]]
    for wl, mode in runs:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", wl,
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
        if out_path:                                     # (kept after every run: a later child that fails loses nothing)
            with open(out_path + ".partial", "w") as f:
                json.dump(results, f)
    summary = {}
    spread = lambda v: 100.0 * (max(v) / min(v) - 1.0)
    for wl in SYSTEMS:
        of = lambda m: [r for r in results if r["workload"] == wl and r["mode"] == m]
        row = {"atoms": of("nve")[0]["atoms"]}
        for m in modes:
            if m != "reads":
                v = [r["ms_per_step"] for r in of(m)]
                row[m + "_ms"], row[m + "_all_ms"], row[m + "_spread_percent"] = min(v), sorted(round(x, 4) for x in v), spread(v)
        if parent:
            row["nve_against_parent_percent"] = 100.0 * (row["nve_ms"] / row["nve_parent_ms"] - 1.0)
        cs = [r["cases"]["cna"] for r in of("reads")]
        mine, theirs = [c["read_ms"] for c in cs], [c["coord_read_ms"] for c in cs]
        c = dict(cs[0], read_ms=min(mine), read_all_ms=sorted(round(x, 4) for x in mine), read_spread_percent=spread(mine))
        c["coord_read_ms"], c["coord_read_all_ms"] = min(theirs), sorted(round(x, 4) for x in theirs)
        c["read_over_coord"] = c["read_ms"] / c["coord_read_ms"]
        c["read_in_nve_steps"] = c["read_ms"] / row["nve_ms"]
        c["centres_per_second"] = row["atoms"] / (c["read_ms"] * 1e-3)
        row["cases"] = {"cna": c}
        summary[wl] = row
        print(wl, json.dumps(row))
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"steps": steps, "warmup": warmup, "reps": REPS, "reads_timed": READS, "summary": summary, "results": results}, f, indent=1)
        os.remove(out_path + ".partial")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
