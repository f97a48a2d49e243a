"""Cost of the device minimiser: ms per FIRE iteration (mdp_fire_iterate) against ms per NVE step of the resident C-ABI
path (mdp_md_integrate_check with the fused final half, as bench.py drives it) OF THE PARENT COMMIT'S LIBRARY, on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms), jittered by 0.05 A
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si), jittered by 0.05 A
and, for REBO-MoS, against the same relaxation through the host-mode path: mdp_rebomos_compute_host per iteration
(positions up, forces down) with the FIRE arithmetic in NumPy on the host (tests/fireref.py).
Every (system, mode) runs in a process of its own under `timeout -k 10`, REPS times, the modes alternating; the fastest
run of each counts.  Both device modes start from rest from the same jittered positions and reneighbour by the on-device
check; the builds of each run are recorded.  The parent stops at the first child that does not end cleanly.
Usage: MDP_PARENT_LIB=/path/to/parent/libmdpair_hip.so python profiles/fire_mdp_rate.py [out.json] [--steps K] [--warmup W]
(without MDP_PARENT_LIB the NVE steps run on this tree's library, and the result says so)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = {"rebomos": (24, 24, 24), "aeam": (63, 63, 63)}
REPS = 2
EXPECTED = 5.0   # per cent over the parent's NVE step beyond which DESIGN.md owes an explanation (not a gate)


def child(workload, mode, steps, warmup):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
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
    s = S.jitter(s, 0.05, seed=11)
    out = {"workload": workload, "mode": mode, "atoms": s.n, "steps": steps,
           "library": "the parent commit's (MDP_PARENT_LIB)" if os.environ.get("MDP_LIB_PATH") else "this tree"}
    if mode == "hostfire":
        # host mode: the host owns x and v, the device only computes (what LAMMPS' own minimize drives a pair style through)
        import fireref
        x_all, type_all, tag_all, owner, shift, nlocal, nghost = S.with_ghosts(s, cutghost)
        ctx.set_atoms_host(nlocal, x_all, type_all, tag_all, len(s.mass) - 1, map_)
        ctx.set_skin(skin)

        def fe(x):
            xa = np.concatenate([x, x[owner] + shift])
            ctx.set_positions_host(xa)
            return ctx.rebomos_compute_host(nlocal, eflag=0, vflag=0)["f"], 0.0
        fire = fireref.Fire(x_all[:nlocal], s.mass[s.type], 0.001, S.FTM2V)
        f, _ = fe(fire.x)
        for _ in range(warmup):
            fire.advance(f)
            f, _ = fe(fire.x)
        t0 = time.perf_counter()
        for _ in range(steps):
            fire.advance(f)
            f, _ = fe(fire.x)
        out["ms_per_step"] = (time.perf_counter() - t0) * 1e3 / steps
        out["fnorm"] = float(np.sqrt((f * f).sum()))
        print("RESULT " + json.dumps(out), flush=True)
        return
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_)
    d.compute(1, 0)
    if mode == "fire":
        ctx.fire_setup(0.0, 0.0, 10 ** 9, 10 ** 9)
        ctx.fire_iterate(warmup)
        ctx.sync()
        torch.cuda.synchronize()
        r0 = ctx.dd_info()["reneighbors"]
        t0 = time.perf_counter()
        ctx.fire_iterate(steps)
        ctx.sync()
        out["ms_per_step"] = (time.perf_counter() - t0) * 1e3 / steps
        st = ctx.fire_state()
        out.update(builds=ctx.dd_info()["reneighbors"] - r0, fnorm=st["fnorm"], fnorm_initial=st["fnorm_initial"],
                   late=st["late"], negatives=st["negatives"])
    else:
        def run(n):
            for k in range(1, n + 1):
                d.step(0, 0, rebuild="auto", defer_final=k < n)
        run(warmup)
        d.flush()
        b0 = d.builds
        torch.cuda.synchronize()
        ctx.sync()
        t0 = time.perf_counter()
        run(steps)
        d.flush()
        ctx.sync()
        out["ms_per_step"] = (time.perf_counter() - t0) * 1e3 / steps
        out.update(builds=d.builds - b0, dangerous=d.dangerous)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 300
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 30
    host_steps = int(args[args.index("--host-steps") + 1]) if "--host-steps" in args else 20
    out_path = next((a for a in args if a.endswith(".json")), None)
    parent = os.environ.get("MDP_PARENT_LIB")
    results = []
    runs = [(wl, mode) for wl in SYSTEMS for _ in range(REPS) for mode in ("nve", "fire")] + [("rebomos", "hostfire")]
    for wl, mode in runs:
        env = dict(os.environ)
        env.pop("MDP_LIB_PATH", None)
        if mode == "nve" and parent:
            env["MDP_LIB_PATH"] = parent
        n, w = (host_steps, 2) if mode == "hostfire" else (steps, warmup)
        cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", wl, mode, str(n), str(w)]
        p = subprocess.run(cmd, capture_output=True, text=True, env=env)
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
        b = min((r for r in results if r["workload"] == wl and r["mode"] == "fire"), key=lambda r: r["ms_per_step"])
        extra = 100.0 * (b["ms_per_step"] / a["ms_per_step"] - 1.0)
        summary[wl] = {"atoms": a["atoms"], "parent_nve_ms": a["ms_per_step"], "fire_ms": b["ms_per_step"], "extra_percent": extra,
                       "builds": [a["builds"], b["builds"]], "nve_library": a["library"], "expected_percent": EXPECTED,
                       "needs_explanation": extra > EXPECTED}
        print(f"{wl}: {a['atoms']} atoms  NVE step ({a['library']}) {a['ms_per_step']:.3f} ms  FIRE iteration {b['ms_per_step']:.3f} ms  "
              f"(+{extra:.2f} %; builds {a['builds']} / {b['builds']})")
    h = [r for r in results if r["mode"] == "hostfire"]
    if h:
        f = summary["rebomos"]["fire_ms"]
        summary["rebomos"]["host_mode_fire_ms"] = h[0]["ms_per_step"]
        summary["rebomos"]["host_mode_over_device"] = h[0]["ms_per_step"] / f
        print(f"rebomos: host-mode FIRE iteration {h[0]['ms_per_step']:.1f} ms = {h[0]['ms_per_step'] / f:.1f} x the device iteration")
    if out_path:
        with open(out_path, "w") as fo:
            json.dump({"steps": steps, "warmup": warmup, "summary": summary, "results": results}, fo, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
