"""Cost of several Langevin baths in the device integrator: ms per step of the resident C-ABI path (mdp_md_integrate_check
with the fused final half, as bench.py drives it) on
  * REBO-MoS bulk, in.rebomos-bulk's cell replicated 24x24x24 (3.98 M atoms) from 300 K
  * the AEAM alloy, fcc a = 4.045 A, 63^3 cells (1.0 M atoms, 0.75 % Si) at 863 K
in one session on one MI355X.  Two questions:
  1. Did any path change against the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH)?
       nve        all-atoms NVE
       lgv_all    one bath on all atoms (mdp_langevin_setup, no mask)
       lgv_third  one bath on the third of the box x < 1/3 (mdp_langevin_group: the MASK kernels)
       union      one bath, `tally yes`, on two strips of a sixth of the box each (x < 1/6 and 1/2 <= x < 2/3)
       two_baths  a hot bath on the first strip and a cold bath on the second, `tally yes` both (mdp_langevin_baths:
                  the LANGEVIN = MDP_LANGEVIN_MAXBATH instantiations, four tally slots per block instead of one)
     each with the parent's library and with this build in alternating processes, REPS of each.  The spread of the parent's
     own repetitions is reported next to the difference: a difference beyond it needs an explanation.
  2. What do two baths cost against one bath over the same atoms?  union and two_baths of this build, which alternate inside
     a process.  The ratio and the spread of its repetitions are reported; no bar is set for it.
A process builds the system once and runs its modes one after the other, each on a fresh context; every process runs
under `timeout -k 10`, and the parent stops at the first one that does not end cleanly.  All modes reneighbor on the same
steps: the alloy at a fixed interval, REBO-MoS by the on-device check (the builds of each run are recorded).
Usage: python profiles/langevin_baths_rate.py [out.json] [--steps K] [--warmup W] [--parent-lib PATH] [--only rebomos|aeam]"""
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
OLD_MODES = ("nve", "lgv_all", "lgv_third")
NEW_MODES = ("union", "two_baths", "union", "two_baths")


def child(workload, modes, steps, warmup):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.load_package()
    import numpy as np
    import torch
    from lammps_plugins_amd.host import capi, resident, system as S
    gold = os.path.join(ROOT, "tests", "golden", "potentials")
    rep = SYSTEMS[workload]
    if workload == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), rep)
        p = capi.read_rebomos_file(os.path.join(gold, "MoS.REBO.set5b"))
    else:
        af = capi.AeamFile(os.path.join(gold, "AlSi.aeam"))
        s = S.fcc_cell(4.045, rep, frac_type2=0.0075, seed=7683797)
        s.mass[1:3] = af.mass[:2]
        tabs = af.build()
    T = TEMPS[workload]
    v0 = S.gaussian_velocities(s, 2.0 * T, seed=1082337)   # (equipartition gives half of it to the lattice)
    lam = s.box.x2lamda(S.wrap(s.box, s.x))[:, 0]
    third = lam < 1.0 / 3.0
    hot, cold = lam < 1.0 / 6.0, (lam >= 0.5) & (lam < 2.0 / 3.0)
    by_tag = np.zeros(int(s.tag.max()) + 1, dtype=np.int32)
    by_tag[s.tag] = 1 | np.where(third, 2, 0) | np.where(hot | cold, 4, 0) | np.where(hot, 8, 0) | np.where(cold, 16, 0)
    every = REBUILD_EVERY[workload]
    for mode in modes:
        ctx = capi.Context(0)
        if workload == "rebomos":
            ctx.rebomos_set_params(p)
            style, skin, map_, cutghost = capi.STYLE_REBOMOS, 2.0, [0, 0, 1], 3.0 * p.rcmax[0][0] + 2.0
        else:
            ctx.aeam_set_tables(tabs)
            style, skin, map_, cutghost = capi.STYLE_AEAM, 1.0, None, float(af.cut_table(tabs).max()) + 1.0
        d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)
        last, bath_atoms = warmup + steps, 0
        if mode == "lgv_all":
            d.langevin(T, T, 0.1, 48271, first=0, last=last)
            bath_atoms = s.n
        elif mode == "lgv_third":
            d.set_group(by_tag, 0, 2)
            d.langevin(T, T, 0.1, 48271, first=0, last=last, natoms=int(third.sum()))
            bath_atoms = int(third.sum())
        elif mode == "union":
            d.set_group(by_tag, 0, 4)
            d.langevin(T, T, 0.1, 48271, tally=True, first=0, last=last, natoms=int((hot | cold).sum()))
            bath_atoms = int((hot | cold).sum())
        elif mode == "two_baths":
            d.set_group(by_tag, 0)
            d.langevin_baths([dict(t_start=1.1 * T, t_stop=1.1 * T, damp=0.1, seed=48271, tally=True, bit=8, natoms=int(hot.sum())),
                              dict(t_start=0.9 * T, t_stop=0.9 * T, damp=0.1, seed=7919, tally=True, bit=16, natoms=int(cold.sum()))],
                             first=0, last=last)
            bath_atoms = int((hot | cold).sum())
        d.compute(1, 0)

        def run(n, k0):
            for k in range(1, n + 1):
                ev = 1 if (k0 + k) % 100 == 0 else 0
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
               "builds": d.builds - b0, "dangerous": d.dangerous, "bath_atoms": bath_atoms,
               "library": "parent" if os.environ.get("MDP_LIB_PATH") else "this build"}
        print("RESULT " + json.dumps(out), flush=True)
        ctx.close()


def main():
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 300
    warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 30
    parent = os.path.abspath(args[args.index("--parent-lib") + 1]) if "--parent-lib" in args else None
    only = args[args.index("--only") + 1] if "--only" in args else None
    out_path = next((a for a in args if a.endswith(".json")), None)
    results = []

    def save(summary=None):   # (after every process: a run that is cut short leaves what it measured)
        if out_path:
            with open(out_path, "w") as f:
                json.dump({"steps": steps, "warmup": warmup, "repetitions": REPS, "summary": summary or {}, "results": results}, f,
                          indent=1)

    for wl in SYSTEMS:
        if only and wl != only:
            continue
        for rep in range(REPS):
            for lib in (("parent", "this") if parent else ("this",)):
                modes = OLD_MODES + NEW_MODES
                cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--child", wl, ",".join(modes),
                       str(steps), str(warmup)]
                env = dict(os.environ)
                env.pop("MDP_LIB_PATH", None)
                if lib == "parent":
                    env["MDP_LIB_PATH"] = parent
                p = subprocess.run(cmd, capture_output=True, text=True, env=env)
                lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or len(lines) != len(modes):
                    print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                    print(f"{wl} {lib} repetition {rep}: exit status {p.returncode}; stopping", file=sys.stderr)
                    sys.exit(1)
                for l in lines:
                    r = json.loads(l[7:])
                    r["repetition"] = rep
                    results.append(r)
                    print(json.dumps(r), flush=True)
                save()
    summary = {}
    for wl in sorted({r["workload"] for r in results}):
        def ms(mode, lib):
            return [r["ms_per_step"] for r in results if r["workload"] == wl and r["mode"] == mode and r["library"] == lib]
        row = {"atoms": next(r["atoms"] for r in results if r["workload"] == wl)}
        for mode in OLD_MODES + NEW_MODES[:2]:
            new = ms(mode, "this build")
            row[mode] = {"this_ms": new, "this_best": min(new)}
            text = f"{wl} {mode}: this build {min(new):.3f} ms/step"
            if parent:
                old = ms(mode, "parent")
                spread = 100.0 * (max(old) - min(old)) / min(old)
                diff = 100.0 * (min(new) / min(old) - 1.0)
                row[mode].update(parent_ms=old, parent_best=min(old), parent_spread_percent=spread, against_parent_percent=diff,
                                 inside_parent_spread=abs(diff) <= spread)
                text += f", parent {min(old):.3f} (its own spread {spread:.2f} %), difference {diff:+.2f} %"
            print(text)
        one, two = ms("union", "this build"), ms("two_baths", "this build")
        ratios = [b / a for a, b in zip(one, two)]             # alternating pairs, in the order they ran
        row["two_baths_against_union"] = {"union_ms": one, "two_baths_ms": two, "ratio_of_best": min(two) / min(one),
                                          "pair_ratios": ratios,
                                          "union_spread_percent": 100.0 * (max(one) - min(one)) / min(one),
                                          "two_baths_spread_percent": 100.0 * (max(two) - min(two)) / min(two)}
        print(f"{wl} two baths against one bath on the union: {min(two):.3f} / {min(one):.3f} ms/step = {min(two) / min(one):.4f} "
              f"(pairs {min(ratios):.4f} .. {max(ratios):.4f}; spreads {row['two_baths_against_union']['union_spread_percent']:.2f} % "
              f"and {row['two_baths_against_union']['two_baths_spread_percent']:.2f} %)")
        summary[wl] = row
    save(summary)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3].split(","), int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
