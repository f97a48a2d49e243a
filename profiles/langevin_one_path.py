"""Bit-for-bit record of the Langevin thermostat's trajectories, for two builds of the library (DESIGN section 4 item 42:
the one-bath and the several-bath code became one set of templates; nothing a run computes may move).

Every case runs once with the PARENT commit's library (--parent-lib PATH, loaded through MDP_LIB_PATH) and once with this
build, each in a process of its own under `timeout -k 10`; the chain stops at the first process that does not end
cleanly.  At every read a case writes the SHA-256 of the raw bytes of x, v and f in tag order and float.hex() of every
tally.  The two records, profiles/langevin_one_path/parent.txt and this.txt, must be byte-identical.  Where only alloy cases
differ the parent's alloy cases run once more (parent_again.txt): the alloy's three-body forces are added with float
atomics, so two runs of ONE library agree to rounding only (tests/test_gpu_langevin_baths.py holds them to 1e-12 A), and a
difference the parent shows against itself says nothing about this build.  REBO-MoS adds everything in a fixed order.

The small cells of tests/test_gpu_langevin_baths.py (REBO-MoS 2x2x1 bulk cells, the 864-atom alloy: more than one 256-atom
block, the last one partial), its masks and baths, 200 steps with rebuild="auto", reads at its EVERY_ODD (a multiple of 14
finds its final half deferred, the others run it on their own):
  a  one bath on all atoms, no mask: ramp, ratio, zero yes, tally yes
  b  one bath on a Langevin group inside an integrate group
  c  the three baths        d  the four baths
  e1 / e3  host-linked (mdp_hnve_*) from shuffled atoms, one bath / the three, reads every 20 steps
  f1 / f2  two mdp_langevin_run calls on one context, the final half of the first run's last step left to the fused kernel of
           the second run's first step by a host that does not tell the library (the need_setup branch of md_launch_advance),
           with one bath / two baths
Usage: python profiles/langevin_one_path.py --parent-lib PATH [--out DIR]"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a", "b", "c", "d", "e1", "e3", "f1", "f2")
STYLES = ("rebomos", "aeam")
NSTEPS, SKIN = 200, 0.5
EVERY_ODD = (7, 14, 21, 49, 98, 133, 140, 161, 200)
EVERY20 = tuple(range(20, 201, 20))
BATHS = (dict(t_start=300.0, t_stop=900.0, damp=0.05, seed=48271, ratio={1: 2.0, 2: 0.5}, zero=True, tally=True),
         dict(t_start=100.0, t_stop=100.0, damp=0.02, seed=7919, ratio=None, zero=False, tally=True),
         dict(t_start=600.0, t_stop=200.0, damp=0.1, seed=48271, ratio=None, zero=True, tally=False),
         dict(t_start=200.0, t_stop=500.0, damp=0.03, seed=104729, ratio=None, zero=True, tally=True))


def child(case, style):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    g.load_package()
    import ctypes as C
    import numpy as np
    from lammps_plugins_amd.host import capi, resident, system as S
    import bathsref
    gold = os.path.join(ROOT, "tests", "golden", "potentials")
    if style == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
        v0 = S.gaussian_velocities(s, 300.0, seed=91)
        p = capi.read_rebomos_file(os.path.join(gold, "MoS.REBO.set5b"))
    else:
        af = capi.AeamFile(os.path.join(gold, "AlSi.aeam"))
        s = S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)
        s.mass[1:3] = af.mass[:2]
        v0 = S.gaussian_velocities(s, 300.0, seed=93)
        tabs = af.build()
    by_tag, grp, groups = bathsref.masks4(s) if case == "d" else bathsref.masks(s)
    GBIT, BITS = bathsref.INTEGRATE_BIT, bathsref.BATH_BITS4 if case == "d" else bathsref.BATH_BITS
    assert -(-s.n // 256) > 1 and s.n % 256

    def dev(k):
        return dict(BATHS[k], bit=BITS[k], natoms=int(groups[k].sum()))

    def record(step, tags, got, tallies):
        order = np.argsort(tags)
        digest = " ".join(f"{k} {hashlib.sha256(np.ascontiguousarray(got[k][order]).tobytes()).hexdigest()}" for k in ("x", "v", "f"))
        print(f"RECORD {case} {style} step {step}: {digest} tally {' '.join(float(e).hex() for e in tallies)}", flush=True)

    ctx = capi.Context(0)
    if style == "rebomos":
        ctx.rebomos_set_params(p)
        dstyle, map_, cut0 = capi.STYLE_REBOMOS, [0, 0, 1], 3.0 * p.rcmax[0][0]
    else:
        ctx.aeam_set_tables(tabs)
        dstyle, map_, cut0 = capi.STYLE_AEAM, None, float(af.cut_table(tabs).max())

    if case in ("e1", "e3"):   # host-linked, as tests/test_gpu_langevin_baths.py drives it
        skin = 2.0 if style == "rebomos" else 1.0
        perm = np.random.default_rng(17).permutation(s.n)
        type_p, tag_p = s.type[perm].copy(), s.tag[perm].copy()
        mask_p, gp = by_tag[tag_p], grp[perm]
        if style == "aeam":
            ctx.aeam_device_lists(True)

        def upload(x, v):
            xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), type_p, tag_p, s.mass), cut0 + skin)
            ctx.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=map_)
            ctx.set_skin(skin)
            ctx.hnve_upload_v(v)

        def compute():
            if style == "rebomos":
                ctx._ck(ctx.L.mdp_rebomos_compute_host(ctx.h, 0, 0, None, None, None, None, None))
            else:
                eng, vir = C.c_double(0.0), np.zeros(6)
                ctx._ck(ctx.L.mdp_aeam_density_host(ctx.h, C.c_int(0), None, None, C.byref(eng), None))
                ctx._ck(ctx.L.mdp_aeam_force_host(ctx.h, C.c_int(0), C.c_int(0), None, None, C.byref(eng), capi._dp(vir), None, None))
        ctx.set_box_host(s.box)
        ctx.hnve_setup(0.001, S.FTM2V, s.mass)
        ctx.integrate_group(GBIT)
        b = BATHS[0]
        if case == "e1":       # the calls of the one thermostat
            ctx.langevin_setup(b["t_start"], b["t_stop"], b["damp"], b["seed"], int(groups[0].sum()), ratio=b["ratio"], zero=b["zero"],
                               tally=b["tally"], boltz=S.BOLTZ, mvv2e=S.MVV2E)
            ctx.langevin_group(BITS[0])
        else:
            cfgs = [dev(k) for k in range(3)]
            for cfg in cfgs:
                cfg["t_period"] = cfg.pop("damp")
            ctx.langevin_baths(cfgs, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        ctx.langevin_run(0, NSTEPS)
        upload(S.wrap(s.box, s.x)[perm].copy(), v0[perm])
        ctx.hnve_set_mask(mask_p)
        compute()
        for step in range(1, NSTEPS + 1):
            moved, late = ctx.hnve_initial()
            if moved or step % 50 == 0:
                got = ctx.hnve_download(s.n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]
                upload(xw, got["v"])
                ctx.hnve_set_mask(mask_p)
            compute()
            ctx.hnve_final()
            if step in EVERY20:
                e = [ctx.langevin_tally(bath=k) for k in range(3)] if case == "e3" else [ctx.langevin_tally()]
                record(step, tag_p, ctx.hnve_download(s.n, want=("x", "v", "f")), e)
        ctx.close()
        return

    d = resident.DeviceDomain(ctx, dstyle, s, cut0 + SKIN, SKIN, map_, v0=v0)
    b, last, ntally = BATHS[0], NSTEPS // 2 if case in ("f1", "f2") else NSTEPS, 0
    if case == "a":
        d.langevin(b["t_start"], b["t_stop"], b["damp"], b["seed"], ratio=b["ratio"], zero=True, tally=True, first=0, last=last)
    elif case in ("b", "f1"):
        d.set_group(by_tag, GBIT, BITS[0])
        d.langevin(b["t_start"], b["t_stop"], b["damp"], b["seed"], ratio=b["ratio"], zero=True, tally=True, first=0, last=last,
                   natoms=int(groups[0].sum()))
    else:
        ntally = {"c": 3, "d": 4, "f2": 2}[case]
        d.set_group(by_tag, GBIT)
        d.langevin_baths([dev(k) for k in range(ntally)], first=0, last=last)
    d.compute(1, 0)

    def read(step):
        e = [d.langevin_tally(bath=k) for k in range(ntally)] if ntally else [d.langevin_tally()]
        d.flush()
        record(step, d.tags_local, ctx.md_download(d.nlocal, want=("x", "v", "f")), e)

    if case in ("f1", "f2"):
        # no step tells the library of a deferred final half (mdp_md_defer_final is never called on this context), so the
        # fused kernel behind the second mdp_langevin_run finds with_final and need_setup together
        assert last not in EVERY_ODD
        for step in range(1, NSTEPS + 1):
            if step == last:
                ctx.md_defer_final = lambda: None     # (the last final half of run 1 is left to the next step's kernel ...)
                d.step(0, 0, rebuild="auto", defer_final=True)
                del ctx.md_defer_final
                ctx.langevin_run(last, NSTEPS)        # (... across the second run's set-up, which cannot complete it)
                continue
            d.step(0, 0, rebuild="auto", defer_final=False)
            if step in EVERY_ODD:
                read(step)
        ctx.close()
        return
    for step in range(1, NSTEPS + 1):
        ev = step in EVERY_ODD
        d.step(1 if ev else 0, 0, rebuild="auto", defer_final=(not ev) or step % 14 == 0)
        if ev:
            read(step)
    ctx.close()


def main():
    args = sys.argv[1:]
    parent = os.path.abspath(args[args.index("--parent-lib") + 1])
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "langevin_one_path")
    os.makedirs(out, exist_ok=True)

    def runs(lib, name, styles):
        lines = []
        for case in CASES:
            for style in styles:
                env = dict(os.environ)
                env.pop("MDP_LIB_PATH", None)
                if lib == "parent":
                    env["MDP_LIB_PATH"] = parent
                p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", case, style],
                                   capture_output=True, text=True, env=env)
                got = [l[7:] for l in p.stdout.splitlines() if l.startswith("RECORD ")]
                if p.returncode != 0 or not got:
                    print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                    print(f"{lib} {case} {style}: exit status {p.returncode}; stopping", file=sys.stderr)
                    sys.exit(1)
                lines += got
                print(f"{lib} {case} {style}: {len(got)} reads", flush=True)
        with open(os.path.join(out, name), "w") as f:
            f.write("\n".join(lines) + "\n")
        return lines

    old, new = runs("parent", "parent.txt", STYLES), runs("this", "this.txt", STYLES)
    differ = sorted({" ".join(a.split()[:2]) for a, b in zip(old, new) if a != b})
    print("parent.txt and this.txt are byte-identical" if old == new else f"parent.txt and this.txt DIFFER in {differ}")
    if old != new and all(d.endswith("aeam") for d in differ):
        # the alloy's three-body forces are summed with float atomics: is the parent's library equal to ITSELF there?
        again = runs("parent", "parent_again.txt", ("aeam",))
        first = [l for l in old if l.split()[1] == "aeam"]
        print("the parent's alloy runs repeat bit for bit: the difference is this build's" if again == first else
              "the parent's alloy runs differ from THEMSELVES in " + str(sorted({" ".join(a.split()[:2]) for a, b in zip(first, again) if a != b})))
    sys.exit(0 if old == new else 1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
