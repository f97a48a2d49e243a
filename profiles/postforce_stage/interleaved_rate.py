"""The children of profiles/indent_mdp_rate.py and profiles/spring_mdp_rate.py (one process per run, NVE and the stage on),
run alternately from a checkout of the parent commit and from this one: parent, this, parent, this ... for every (script,
system, mode), so that a drift of the machine over tens of seconds reaches both sides alike.  The three-block order
parent / this / parent of the same scripts cannot tell such a drift from a difference of the code.
Usage: python profiles/postforce_stage/interleaved_rate.py <checkout of the parent commit, built> out.json [--reps R]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    parent, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 4
    env = dict(os.environ)
    env.pop("MDP_LIB_PATH", None)
    runs, rows = {}, []
    for kind in ("indent", "spring"):
        for wl in ("rebomos", "aeam"):
            for mode in ("nve", kind):
                for rep in range(reps):
                    for side, tree in (("parent", parent), ("this", ROOT)):
                        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(tree, "profiles", kind + "_mdp_rate.py"),
                               "--child", wl, mode, "300", "30"]
                        p = subprocess.run(cmd, capture_output=True, text=True, env=env)
                        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                        if p.returncode != 0 or not lines:
                            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                            print(f"{kind} {wl} {mode} {side}: exit status {p.returncode}; stopping", file=sys.stderr)
                            sys.exit(1)
                        ms = json.loads(lines[-1][7:])["ms_per_step"]
                        runs.setdefault((kind, wl, mode, side), []).append(ms)
                        print(f"{kind} {wl} {mode} {side} {ms:.4f}", flush=True)
                a, b = runs[(kind, wl, mode, "parent")], runs[(kind, wl, mode, "this")]
                rows.append({"script": kind, "system": wl, "mode": mode, "parent_ms": [round(x, 4) for x in a], "this_ms": [round(x, 4) for x in b],
                             "parent_min_max": [round(min(a), 4), round(max(a), 4)], "this_best": round(min(b), 4),
                             "this_best_inside_the_parents_runs": min(b) <= max(a)})
                print(json.dumps(rows[-1]), flush=True)
    with open(out_path, "w") as f:
        json.dump({"steps": 300, "warmup": 30, "reps": reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
