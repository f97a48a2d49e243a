"""What a heat-current sample costs in resident mode, and that a run without one is undisturbed: ms per step of the resident
C-ABI path (mdp_md_integrate_check with the fused final half, as bench.py drives it) on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
in three modes on the same MI355X:
  (a) nve_parent  NVE with the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH)
  (b) nve         NVE with this build and no per-atom tally: accepted when (b) - (a) lies inside the spread of (a)'s own
                  repetitions in this session (both spreads are recorded)
  (c) sample      this build with a tallying step (eflag 3, vflag 5: the rebomos per-atom-virial centre path, the aeam CSR
                  kernels) and a read of J (DeviceDomain.heatflux) every 10 steps -- a Green-Kubo sampling cadence.  Then, in
                  the same process: SAMPLES tallying steps on their own, each between two device synchronisations, against
                  as many plain steps timed the same way ("k plain steps per sample"), and READS blocking reads of
                  mdp_heatflux_sums on their own, next to the bandwidth estimate of about 100 bytes per atom (v 24, m 8,
                  eatom 8, vatom 48, partial sums).
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating and their order
rotating from one repetition to the next; the fastest run of each counts and every run is kept in the JSON.  All modes
reneighbor on the same steps: the alloy at a fixed interval (REBUILD_EVERY), REBO-MoS by the on-device check.  The parent
stops at the first child that does not end cleanly.
Usage: python profiles/heatflux_mdp_rate.py [out.json] [--steps K] [--warmup W] [--reps R] [--parent-lib PATH]"""
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
READS = 20
SAMPLES = 5
SAMPLE_EVERY = 10
BYTES_PER_ATOM = 100.0
MODES = ("nve_parent", "nve", "sample")


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
    d.compute(1, 0)
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps,
           "library": "the parent commit's (--parent-lib)" if os.environ.get("MDP_LIB_PATH") else "this build"}
    thermo = 100
    every = REBUILD_EVERY[workload]
    sampling = mode == "sample"

    def run(n, k0):
        for k in range(1, n + 1):
            tally = sampling and (k0 + k) % SAMPLE_EVERY == 0
            ev = 1 if (k0 + k) % thermo == 0 else 0
            rebuild = "auto" if not every else (k0 + k) % every == 0
            if tally:
                d.step(3, 5, rebuild=rebuild)
                d.heatflux()
            else:
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
    if sampling:
        def timed(eflag, vflag):
            best = []
            for _ in range(SAMPLES):
                ctx.sync()
                t0 = time.perf_counter()
                d.step(eflag, vflag, rebuild=False)
                ctx.sync()
                best.append((time.perf_counter() - t0) * 1e3)
            return best
        plain, tally = timed(0, 0), timed(3, 5)
        out.update({"plain_step_ms": min(plain), "tally_step_ms": min(tally), "plain_steps_ms": plain, "tally_steps_ms": tally})
        J = d.heatflux()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(READS):
            sums = ctx.heatflux_sums()
        out["read_ms"] = (time.perf_counter() - t0) * 1e3 / READS
        assert int(sums[6]) == s.n
        out.update({"reads_timed": READS, "J": [float(v) for v in J],
                    "read_GBps_at_100B_per_atom": BYTES_PER_ATOM * s.n / (out["read_ms"] * 1e-3) / 1e9})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 300
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
        spread = lambda m: 100.0 * (max(r["ms_per_step"] for r in of(m)) / best[m]["ms_per_step"] - 1.0)
        b, c = best["nve"], best["sample"]
        plain, tally = min(r["plain_step_ms"] for r in of("sample")), min(r["tally_step_ms"] for r in of("sample"))
        read = min(r["read_ms"] for r in of("sample"))
        row = {"atoms": b["atoms"], "nve_ms": b["ms_per_step"], "nve_spread_percent": spread("nve"),
               "all_runs_ms": {m: sorted(round(r["ms_per_step"], 4) for r in of(m)) for m in modes},
               "sample_every_10_ms": c["ms_per_step"], "sample_every_10_extra_percent": 100.0 * (c["ms_per_step"] / b["ms_per_step"] - 1.0),
               "plain_step_ms": plain, "tally_step_ms": tally, "plain_steps_per_sample": tally / plain,
               "read_ms": read, "read_GBps_at_100B_per_atom": BYTES_PER_ATOM * b["atoms"] / (read * 1e-3) / 1e9,
               "builds": {m: best[m]["builds"] for m in modes}}
        text = f"{wl}: {b['atoms']} atoms  NVE {b['ms_per_step']:.3f} (spread {row['nve_spread_percent']:.2f} %)"
        if parent:
            a = best["nve_parent"]
            row["nve_parent_ms"], row["nve_parent_spread_percent"] = a["ms_per_step"], spread("nve_parent")
            row["nve_against_parent_percent"] = 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0)
            row["run_undisturbed"] = row["nve_against_parent_percent"] <= max(row["nve_parent_spread_percent"], 0.5)
            text += f"  parent {a['ms_per_step']:.3f} (spread {row['nve_parent_spread_percent']:.2f} %), {row['nve_against_parent_percent']:+.2f} %"
        text += (f"  a sample every {SAMPLE_EVERY} steps {c['ms_per_step']:.3f} ms/step ({row['sample_every_10_extra_percent']:+.1f} %); a tallying step "
                 f"{tally:.3f} ms = {row['plain_steps_per_sample']:.2f} plain steps of {plain:.3f} ms; a read {read:.4f} ms "
                 f"({row['read_GBps_at_100B_per_atom']:.0f} GB/s at 100 B per atom); builds {row['builds']}")
        summary[wl] = row
        print(text)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"steps": steps, "warmup": warmup, "reps": reps, "sample_every": SAMPLE_EVERY, "summary": summary, "results": results}, f, indent=1)
    if parent and not all(row["run_undisturbed"] for row in summary.values()):
        print("NVE with this build is outside the spread of the parent library's own repetitions: a finding", file=sys.stderr)
        sys.exit(2)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
