"""What `compute profile/mdp` costs, and that the run itself is undisturbed: ms per step of the resident C-ABI path
(mdp_md_integrate_check with the fused final half, as bench.py drives it) on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
in three modes on the same MI355X:
  (a) nve_parent  NVE with the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH)
  (b) nve         NVE with this build and no profile: the step path was not touched, so (b) must equal (a) within the
                  box-to-box spread of the README (2-3 %); anything outside it is a finding to explain
  (c) profile     this build with a profile of 200 bins along z read every 100 steps (DeviceDomain.profile_read: the range
                  pass, the exponents, the sums pass, two blocking downloads); then READS blocking reads on their own, for
                  z:200 (the table in LDS) and for 32 x 32 x 32 (32 768 rows: straight into the global table), timed with a
                  host clock around calls that end in a device synchronise.  No target: what a read costs is recorded, in ms,
                  in NVE steps and as the overhead per step when read every 100 steps; from bytes alone two passes over about
                  68 B per atom (x 32, v 24, m 8, twice v and m) are a few tenths of a millisecond at 3.98 M atoms.
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating and their order
rotating from one repetition to the next (the box is shared: whichever mode runs first in a repetition must not always be
the same one); the fastest run of each counts, the median of each is reported next to it, and every run is kept in the
JSON.  All modes reneighbor on the same steps: the alloy at a fixed interval (REBUILD_EVERY), REBO-MoS by the on-device
check (the builds of each mode are recorded).  The parent stops at the first child that does not end cleanly.
Usage: python profiles/profile_mdp_rate.py [out.json] [--steps K] [--warmup W] [--reps R] [--parent-lib PATH]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = {"rebomos": (24, 24, 24), "aeam": (63, 63, 63)}
TEMPS = {"rebomos": 300.0, "aeam": 863.0}
REBUILD_EVERY = {"rebomos": 0, "aeam": 10}   # 0: the deferred on-device `check yes`
REPS = 6
READS = 10
SPREAD = 3.0   # per cent: (b) against (a)
MODES = ("nve_parent", "nve", "profile")
GRID_RUN = ((2,), (200,))
GRID_BIG = ((0, 1, 2), (32, 32, 32))


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
    v0 = S.gaussian_velocities(s, 2.0 * TEMPS[workload], seed=1082337)   # (equipartition gives half of it to the lattice)
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)
    if mode == "profile":
        d.profile(*GRID_RUN)
    d.compute(1, 0)
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps, "grid": list(GRID_RUN[1]),
           "library": "the parent commit's (--parent-lib)" if os.environ.get("MDP_LIB_PATH") else "this build"}
    thermo = 100
    every = REBUILD_EVERY[workload]

    def run(n, k0):
        for k in range(1, n + 1):
            ev = 1 if (k0 + k) % thermo == 0 else 0
            rebuild = "auto" if not every else (k0 + k) % every == 0
            d.step(ev, 0, rebuild=rebuild, defer_final=not ev and k < n)
            if ev and mode == "profile":
                d.profile_read()

    run(warmup, 0)
    d.flush()
    if mode == "profile":
        d.profile_read()                   # (the table exists before the timed window)
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
    if mode == "profile":
        for key, grid in (("read_ms", GRID_RUN), ("read_big_ms", GRID_BIG)):
            d.profile(*grid)
            d.profile_read()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(READS):
                count, sums, ex = d.profile_read()
            out[key] = (time.perf_counter() - t0) * 1e3 / READS
            assert int(count.sum()) == s.n
            # the two device passes alone, without the exponents' host arithmetic and the table's download
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(READS):
                ctx.profile_range()
            out[key.replace("read", "range")] = (time.perf_counter() - t0) * 1e3 / READS
            mv2 = float(sums[:, 4].astype(float).sum()) * 2.0 ** -int(ex[4])
            out[key.replace("_ms", "_temp")] = mv2 * S.MVV2E / (3.0 * s.n * S.BOLTZ)
        out.update({"reads_timed": READS, "grid_big": list(GRID_BIG[1]), "exponents": [int(e) for e in ex]})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 600
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 30
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else REPS
    parent = os.path.abspath(args[args.index("--parent-lib") + 1]) if "--parent-lib" in args else None
    out_path = next((a for a in args if a.endswith(".json")), None)
    modes = [m for m in MODES if m != "nve_parent" or parent]
    results = []
    runs = [(wl, mode) for wl in SYSTEMS for rep in range(reps) for mode in modes[rep % len(modes):] + modes[:rep % len(modes)]]
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
        of = lambda m: [r for r in results if r["workload"] == wl and r["mode"] == m]
        best = {m: min(of(m), key=lambda r: r["ms_per_step"]) for m in modes}
        b, c = best["nve"], best["profile"]
        read, big = min(r["read_ms"] for r in of("profile")), min(r["read_big_ms"] for r in of("profile"))
        row = {"atoms": b["atoms"], "nve_ms": b["ms_per_step"],
               "all_runs_ms": {m: sorted(round(r["ms_per_step"], 4) for r in of(m)) for m in modes},
               "profile_every_100_ms": c["ms_per_step"],
               "profile_every_100_extra_percent": 100.0 * (c["ms_per_step"] / b["ms_per_step"] - 1.0),
               "read_ms": read, "read_in_nve_steps": read / b["ms_per_step"], "read_big_ms": big,
               "range_ms": min(r["range_ms"] for r in of("profile")), "builds": {m: best[m]["builds"] for m in modes}}
        text = f"{wl}: {b['atoms']} atoms  NVE {b['ms_per_step']:.3f}"
        if parent:
            a = best["nve_parent"]
            med = lambda m: statistics.median(r["ms_per_step"] for r in of(m))
            row["nve_parent_ms"] = a["ms_per_step"]
            row["nve_against_parent_percent"] = 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0)
            row["nve_median_ms"], row["nve_parent_median_ms"] = med("nve"), med("nve_parent")
            row["nve_against_parent_median_percent"] = 100.0 * (med("nve") / med("nve_parent") - 1.0)
            row["spread_percent"] = SPREAD
            row["run_undisturbed"] = abs(row["nve_against_parent_percent"]) <= SPREAD
            text += (f" (parent {a['ms_per_step']:.3f}, {row['nve_against_parent_percent']:+.2f} %; medians {row['nve_median_ms']:.3f} / "
                     f"{row['nve_parent_median_ms']:.3f}, {row['nve_against_parent_median_percent']:+.2f} %)")
        text += (f"  with a read every 100 steps {c['ms_per_step']:.3f} ({row['profile_every_100_extra_percent']:+.2f} %) ms/step; a read of "
                 f"z:200 {read:.3f} ms = {row['read_in_nve_steps']:.2f} steps (its range pass {row['range_ms']:.3f} ms), of 32x32x32 {big:.3f} ms; "
                 f"builds {row['builds']}")
        summary[wl] = row
        print(text)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"steps": steps, "warmup": warmup, "reps": reps, "grid": list(GRID_RUN[1]), "grid_big": list(GRID_BIG[1]),
                       "summary": summary, "results": results}, f, indent=1)
    if parent and not all(row["run_undisturbed"] for row in summary.values()):
        print("NVE with this build is outside the spread of the parent library: a finding", file=sys.stderr)
        sys.exit(2)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
