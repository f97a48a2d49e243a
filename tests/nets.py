"""The randomised parity nets: one home for what profiles/*_fuzz.py run by hand and tests/test_gpu_nets.py runs at fixed
seeds.  A helper module like fixture_cases.py, not a test module.

For each net NAME of NETS:
  draw_NAME(rng) -> spec      pure Python (no GPU, no oracle): one case drawn from a random.Random, the draws consumed in
                              the order the command-line nets have always used, so `profiles/NAME_fuzz.py <cases> <seed>`
                              still draws the cases recorded under profiles/r06_NAME/;
  run_NAME(spec) -> (errors, limits)
                              builds and runs the case on the GPU; the case passes when errors[q] < limits[q] for every
                              q of limits (a condition that must hold counts 0 when it does, 1 when it does not; errors
                              may carry more keys, which only the report prints);
  line_NAME(spec, errors)     the report line of the case.

spec["env"] holds the library's environment knobs of the case (MDP_INNER_SKIN, MDP_PRUNE, MDP_LJ_QUEUE,
MDP_PRUNE_BUFFER, MDP_MEASURE_GRID).  A case runs with exactly these set and the others unset: the caller applies them (knobs() here,
monkeypatch under pytest); run_NAME never writes os.environ.  spec["id"] is the short text of a test id."""
from __future__ import annotations

import atexit
import contextlib
import os
import random
import tempfile

import numpy as np

from lammps_plugins_amd.host import system as S

KNOBS = ("MDP_INNER_SKIN", "MDP_PRUNE", "MDP_LJ_QUEUE", "MDP_PRUNE_BUFFER", "MDP_MEASURE_GRID")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lammps-plugins_amd")

# The fixed seeds of the GPU suite: net -> [(seed, cases)].  tests/test_net_draws.py asserts that they reach the corners
# the nets exist for.
SUITE = {
    "force": [(1, 60)],
    "hostmode_walk": [(1, 30)],
    "aeam_types": [(1, 30)],
    "prune": [(1, 10)],
    "dd": [(1, 10)],
    "hnve": [(1, 8)],
    "minilmp": [(2, 6)],
    "trajectory": [(1, 12)],
    "block": [(1, 8)],
    "fire": [(4, 16)],
    "langevin": [(42, 14)],
    "heat": [(2, 12)],
    "measure": [(4, 16)],
    "peratom": [(27, 16)],
    "structure": [(1018, 16)],
    "postforce": [(44, 16)],
}


def cases(net, seed, ncase):
    """the first ncase specs of `net` at `seed`, as the command-line net draws them"""
    rng = random.Random(seed)
    return [NETS[net][0](rng) for _ in range(ncase)]


@contextlib.contextmanager
def knobs(env):
    """the library's knobs of one case set (and the others unset) for the duration of the block; restored after"""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def passed(errors, limits):
    return all(errors[q] < limits[q] for q in limits)


_R = {}


def _res():
    """oracle, parameters and tables, loaded once per process"""
    if not _R:
        from conftest import POT_AEAM, POT_REBOMOS
        from lammps_plugins_amd.host import capi
        import oracle_bindings as ob
        orc = ob.load()
        af = capi.AeamFile(POT_AEAM)
        _R.update(orc=orc, P=orc.rebomos_params(POT_REBOMOS), T=orc.aeam_pot(POT_AEAM), rp=capi.read_rebomos_file(POT_REBOMOS),
                  af=af, tabs=af.build(), pot_aeam=POT_AEAM)
    return _R


def close_shared():
    """close the context the REBO-MoS force cases share (tests/test_gpu_nets.py: at the end of its module; the command
    line: at exit)"""
    ctx = _R.pop("rctx", None)
    if ctx is not None:
        ctx.close()


def _fold(a, owner, n):
    out = a[:n].copy()
    np.add.at(out, owner, a[n:])
    return out


def _inner(rng, choices):
    """the nets' draw of MDP_INNER_SKIN: set (one of choices) in half of the cases"""
    return {"MDP_INNER_SKIN": str(rng.choice(choices))} if rng.random() < 0.5 else {}


def _fmt(v):
    return f"{v:.1e}" if isinstance(v, float) or hasattr(v, "dtype") else f"{v}"


REBO_CELL_N = 288     # atoms of S.rebomos_bulk_cell()


def _rebo_n(rep):
    return REBO_CELL_N * (1 if rep is None else rep[0] * rep[1] * rep[2])


# ---------------------------------------------------------------------------------------------------------------- force
# Random MoS2 cells (scale 0.92-1.16, jitter up to 0.25 A, small replicas) and random Al-Si alloys (4-7 fcc cells,
# 0-50 % Si, jitter up to 0.3 A, half of them in a sheared box) through the host-mode HIP path (device-built or host
# CSR lists, every tally on, then a force-only call) against a LIVE oracle compute on the same inputs.
def draw_force(rng):
    style = rng.choice(["rebomos", "aeam"])
    if style == "rebomos":
        fac, amp, sd = rng.uniform(0.92, 1.16), rng.uniform(0.0, 0.25), rng.randrange(10**6)
        rep = rng.choice([None, (2, 1, 1), (1, 2, 1), (2, 2, 1), (1, 1, 2)])
        spec = dict(style=style, fac=fac, amp=amp, seed=sd, rep=rep, n=_rebo_n(rep))
        desc = f"fac {fac:.3f} amp {amp:.3f} seed {sd} rep {rep}"
    else:
        nc, frac, amp, sd = rng.choice([4, 5, 6, 7]), rng.choice([0.0, 0.0075, 0.03, 0.08, 0.2, 0.5]), rng.uniform(0.0, 0.3), rng.randrange(10**6)
        spec = dict(style=style, cells=nc, frac=frac, amp=amp, seed=sd, tilt=None, n=4 * nc ** 3)
        desc = f"cells {nc} frac {frac} amp {amp:.3f} seed {sd}"
        if rng.random() < 0.5:   # a sheared (triclinic) box: same lamda coordinates in a tilted cell
            L = 4.045 * nc
            spec["tilt"] = [rng.uniform(-0.12, 0.12) * L for _ in range(3)]
            desc += f" tilt {np.round(np.array(spec['tilt']), 2).tolist()}"
    spec["lists"] = rng.choice(["device", "host_csr"])
    spec.update(desc=desc + f" lists {spec['lists']}", env={}, id=f"{style}-{spec['lists']}-n{spec['n']}")
    return spec


def run_force(spec):
    import fixture_cases as FC
    import oracle_bindings as ob
    from lammps_plugins_amd.host import capi
    R = _res()
    if spec["style"] == "rebomos":
        if "rctx" not in R:   # (one context for every REBO-MoS case, as the command-line net has always run them)
            R["rctx"] = capi.Context(0)
            atexit.register(close_shared)
            R["rctx"].rebomos_set_params(R["rp"])
        rctx = R["rctx"]
        s = FC._rebomos(spec["fac"], spec["amp"], spec["seed"], spec["rep"])
        eng = FC.engine("rebomos", s, R["orc"], P=R["P"])
        want = FC.oracle_outputs("rebomos", eng, s.x)
        xa = eng.all_positions(s.x)
        rctx.set_atoms_host(eng.nlocal, xa, eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
        if spec["lists"] == "device":
            rctx.set_skin(2.0)
        else:
            rctx.set_neighbors_csr_host(eng.nn, eng.off, eng.nb, 2.0)
        g = rctx.rebomos_compute_host(eng.nlocal, eflag=3, vflag=5)
        g0 = rctx.rebomos_compute_host(eng.nlocal, eflag=0, vflag=0)
        fs = max(1.0, float(np.abs(want["f"]).max()))
        err = dict(f=np.abs(g["f"] - want["f"]).max() / fs, f0=np.abs(g0["f"] - want["f"]).max() / fs,
                   e=abs(g["eng"] - float(want["eng"])) / abs(float(want["eng"])), ea=np.abs(g["eatom"] - want["eatom"]).max(),
                   va=np.abs(g["vatom"] - want["vatom"]).max() / max(1.0, np.abs(want["vatom"]).max()))
        return err, dict(f=1e-9, f0=1e-9, e=1e-10, ea=1e-9, va=1e-9)
    s = FC._aeam_cell(spec["cells"], spec["frac"], spec["amp"], spec["seed"])
    if spec["tilt"] is not None:
        nb = S.Box(s.box.lo.copy(), s.box.prd.copy(), np.array(spec["tilt"]))
        s = S.System(nb, nb.lamda2x(s.box.x2lamda(s.x)), s.type, s.tag, s.mass)
    eng = FC.engine("aeam", s, R["orc"], T=R["T"])
    want = FC.oracle_outputs("aeam", eng, s.x)
    ctx = capi.Context(0)
    try:
        ctx.aeam_set_tables(R["tabs"])
        if spec["lists"] == "device":
            cut = float(R["af"].cut_table(R["tabs"]).max()) + 1.0
            xa, type_all, tag_all, owner, _, nloc, _ = S.with_ghosts(s, cut)
            ctx.aeam_device_lists(True)
            ctx.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=None)
            ctx.set_skin(1.0)
        else:
            xa, owner, nloc = eng.all_positions(s.x), eng.owner, eng.nlocal
            ctx.set_atoms_host(nloc, xa, eng.type_all, eng.tag_all, 2, map_=None)
            ctx.set_neighbors_csr_host(eng.nn, eng.off, eng.nb, 1.0)
        d = ctx.aeam_density_host(nloc, eflag=3)
        r = ctx.aeam_force_host(len(xa), nloc, np.concatenate([d["fp"], d["fp"][owner]]), eflag=3, vflag=5)
        d0 = ctx.aeam_density_host(nloc, eflag=0)
        r0 = ctx.aeam_force_host(len(xa), nloc, np.concatenate([d0["fp"], d0["fp"][owner]]), eflag=0, vflag=0)
    finally:
        ctx.close()
    fs = max(1.0, float(np.abs(want["f"]).max()))
    err = dict(f=np.abs(ob.fold_ghost_forces(r["f"], owner, nloc) - want["f"]).max() / fs,
               f0=np.abs(ob.fold_ghost_forces(r0["f"], owner, nloc) - want["f"]).max() / fs,
               e=abs(d["eng"] + r["eng"] - float(want["eng"])) / abs(float(want["eng"])),
               ea=np.abs(d["eatom"] + r["eatom"] - want["eatom"]).max(),
               va=np.abs(_fold(r["vatom"], owner, nloc) - want["vatom"]).max() / max(1.0, np.abs(want["vatom"]).max()),
               rho=np.abs(d["rho"] - want["rho"]).max() / max(1.0, np.abs(want["rho"]).max()))
    return err, dict(f=1e-9, f0=1e-9, e=1e-10, ea=1e-9, va=1e-9, rho=1e-11)


def line_force(spec, err):
    return f"{spec['style']} {spec['desc']} n {spec['n']} " + " ".join(f"{q} {_fmt(v)}" for q, v in err.items())


# ---------------------------------------------------------------------------------------------------------- aeam_types
# AEAM runs with 3 - 12 atom types (relabelled copies of the bundled two-element file, tests/aeam_five.py: every new
# element behaves as Al or as Si, so the oracle on the relabelled file is the reference): tile kernels with per-entry
# types for up to 8 types, the generic kernels beyond.  30 device-resident steps, then forces and energy against the
# oracle on the final positions.
def draw_aeam_types(rng):
    nmet, nang = rng.choice([(2, 1), (3, 2), (4, 2), (5, 3), (7, 5), (1, 3), (6, 2)])
    n = rng.choice([6, 8, 10, 12]); frac = rng.choice([0.01, 0.06, 0.25]); temp = rng.choice([300, 863, 2000]); sd = rng.randrange(1, 10**6)
    return dict(nmet=nmet, nang=nang, cells=n, frac=frac, temp=temp, seed=sd, ntypes=nmet + nang, env={},
                id=f"types{nmet}+{nang}-cells{n}-T{temp}")


def run_aeam_types(spec):
    import aeam_five
    import mdref
    from lammps_plugins_amd.host import capi, resident
    R = _res()
    nmet, nang, sd = spec["nmet"], spec["nang"], spec["seed"]
    if "tmp" not in R:
        R["tmp"] = tempfile.mkdtemp()
    path = os.path.join(R["tmp"], f"p{nmet}_{nang}.aeam")
    if not os.path.exists(path):
        aeam_five.write_relabelled_file(path, R["pot_aeam"], [0] * nmet + [1] * nang, ["M%d" % i for i in range(nmet)] + ["X%d" % i for i in range(nang)])
    af = capi.AeamFile(path); T = R["orc"].aeam_pot(path); tabs = af.build()
    s2 = S.jitter(S.fcc_cell(4.045, spec["cells"], frac_type2=spec["frac"], seed=sd), 0.05, seed=sd + 1)
    r = np.random.default_rng(sd)
    ty = np.where(s2.type == 1, r.integers(1, nmet + 1, s2.n), r.integers(nmet + 1, nmet + nang + 1, s2.n)).astype(np.int32)
    s = S.System(s2.box, s2.x.copy(), ty, s2.tag.copy(), np.array([0.0] + list(af.mass)))
    v0 = S.gaussian_velocities(s, float(spec["temp"]), seed=sd + 2)
    ctx = capi.Context(0)
    try:
        ctx.aeam_set_tables(tabs)
        d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, s, float(af.cut_table(tabs).max()) + 1.0, 1.0, None, v0=v0)
        d.compute(0, 0)
        for _ in range(30):
            d.step(0, 0, rebuild="auto")
        d.compute(1, 0)
        th = d.thermo(); got = ctx.md_download(d.nlocal, want=("x", "f")); tags = d.tags_local; builds = d.builds
    finally:
        ctx.close()
    x = np.zeros((s.n, 3)); f = np.zeros((s.n, 3)); x[tags - 1] = got["x"]; f[tags - 1] = got["f"]
    xw = S.wrap(s.box, x)
    o = mdref.AeamCPU(R["orc"], T, S.System(s.box, xw, s.type, s.tag, s.mass)).compute(xw, eflag=1, vflag=0)
    df = float(np.abs(f - o["f_owned"]).max()) / max(1.0, float(np.abs(o["f_owned"]).max())); de = abs(th["pe"] - o["eng"]) / abs(o["eng"])
    return dict(dF=df, dE=de, builds=builds), dict(dF=1e-9, dE=1e-10)


def line_aeam_types(spec, err):
    return (f"types {spec['nmet']}+{spec['nang']} cells {spec['cells']} frac {spec['frac']} T {spec['temp']} seed {spec['seed']} "
            f"dF {err['dF']:.1e} dE {err['dE']:.1e} builds {err['builds']}")


# --------------------------------------------------------------------------------------------------------------- prune
# Dynamic row pruning and the pair queues (one GPU, minihost/ddhost.cpp): random hot / drifting runs with the kernels
# walking PRUNED rows (default) against the same run with MDP_PRUNE=0 (rows as built), against MDP_LJ_QUEUE=1 / 0
# (cubic-branch pairs queued / found by a second walk) and against other inner skins of the style's own lists.  A pair
# missed by the one-step-late displacement trigger shows as a trajectory that leaves its twin.
PRUNE_VARIANTS = (("pruned", {}), ("as_built", {"MDP_PRUNE": "0"}), ("queued", {"MDP_LJ_QUEUE": "1"}), ("walked", {"MDP_LJ_QUEUE": "0"}),
                  ("inner_skin_0.3", {"MDP_INNER_SKIN": "0.3"}), ("inner_skin_1.2", {"MDP_INNER_SKIN": "1.2"}))


def draw_prune(rng):
    style = rng.choice(["rebomos", "aeam"])
    if style == "rebomos":
        rep = rng.choice([(3, 3, 2), (4, 4, 2), (5, 3, 2)]); temp = rng.choice([300, 1500, 3000, 5000]); extra = []
    else:
        n = rng.choice([12, 16, 20]); rep = (n, n, n); temp = rng.choice([300, 863, 2000]); extra = ["-frac2", rng.choice([0.0075, 0.08])]
    drift = [rng.choice([-60, 0, 40, 90]) for _ in range(3)]
    steps = rng.choice([80, 150, 250]); sd = rng.randrange(1, 10**7)
    variants = [(name, env) for name, env in PRUNE_VARIANTS if style == "rebomos" or name in ("pruned", "as_built")]
    return dict(style=style, rep=rep, temp=temp, extra=extra, drift=drift, steps=steps, seed=sd, variants=variants, env={},
                id=f"{style}-T{temp}-steps{steps}")


def run_prune(spec):
    import test_gpu_ddhost as T
    common = ["-style", spec["style"], "-ranks", 1, "-replicate", *spec["rep"], "-steps", spec["steps"], "-thermo", spec["steps"],
              "-temp", spec["temp"], "-seed", spec["seed"], "-drift", *spec["drift"]] + spec["extra"]
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for name, env in spec["variants"]:
            out, _ = T._ddhost(common + ["-dump", os.path.join(d, name)], env=env)
            res[name] = T._dump(os.path.join(d, name), 1) + (out.split("Neighbor list builds = ")[1].split()[0],)
    ref = res["as_built"]
    err, lim = {"builds": res["pruned"][2]}, {}
    for n, r in res.items():
        if n != "as_built":
            err[n + " dx"], err[n + " dv"] = float(np.abs(r[0] - ref[0]).max()), float(np.abs(r[1] - ref[1]).max())
            lim[n + " dx"], lim[n + " dv"] = 1e-9, 1e-8
    return err, lim


def line_prune(spec, err):
    return (f"{spec['style']} rep {spec['rep']} T {spec['temp']} drift {spec['drift']} steps {spec['steps']} seed {spec['seed']} "
            f"{spec['extra']} builds {err.get('builds', '?')} " + " ".join(f"{q} {_fmt(v)}" for q, v in err.items() if q != "builds"))


# ------------------------------------------------------------------------------------------------------------------ dd
# Multi-rank consistency of the C++ resident host (minihost/ddhost.cpp) on one GPU through the RCCL test double: the
# N-rank run must end where the one-rank run ends (positions 1e-8 A, velocities 1e-7 A/ps, thermo rows as printed).
def draw_dd(rng, only=None):
    style = only or rng.choice(["rebomos", "aeam"])
    ranks = rng.choice([2, 3, 4, 6, 8])
    if style == "rebomos":
        rep = rng.choice([(3, 3, 2), (4, 2, 2), (2, 4, 3), (5, 3, 2), (3, 2, 4)])
        temp = rng.choice([300, 900, 1500, 3000, 5000])
        extra = []
    else:
        n = rng.choice([12, 14, 16, 18])
        rep = (n, n, n)
        temp = rng.choice([300, 863, 1200, 3000])
        extra = ["-frac2", rng.choice([0.0, 0.0075, 0.03, 0.08])]
    drift = [rng.choice([-60, -30, 0, 25, 40, 70]) for _ in range(3)]
    steps = rng.choice([40, 60, 90])
    sd = rng.randrange(1, 10**7)
    thermo = rng.choice([steps, 10, 7])     # (energy / virial steps in mid-run: the other kernel variants, sums over ranks)
    return dict(style=style, ranks=ranks, rep=rep, temp=temp, extra=extra, drift=drift, steps=steps, seed=sd, thermo=thermo,
                env={}, id=f"{style}-ranks{ranks}-T{temp}")


def run_dd(spec):
    import test_gpu_ddhost as T
    box = (S.replicate(S.rebomos_bulk_cell(), spec["rep"]) if spec["style"] == "rebomos" else S.fcc_cell(4.045, spec["rep"][0])).box
    common = ["-style", spec["style"], "-replicate", *spec["rep"], "-steps", spec["steps"], "-thermo", spec["thermo"],
              "-temp", spec["temp"], "-seed", spec["seed"], "-drift", *spec["drift"]] + spec["extra"]
    with tempfile.TemporaryDirectory() as d:
        _, rows1 = T._ddhost(["-ranks", 1, "-dump", os.path.join(d, "one")] + common)
        out, rowsn = T._ddhost(["-ranks", spec["ranks"], "-dump", os.path.join(d, "many")] + common, double=True)
        x1, v1 = T._dump(os.path.join(d, "one"), 1)
        xn, vn = T._dump(os.path.join(d, "many"), spec["ranks"])
    dx = xn - x1
    dx -= np.round(box.x2lamda(dx + box.lo)) @ box.h.T
    rows_ok = len(rows1) == len(rowsn) and len(rows1) >= 2
    for a, b in zip(rowsn, rows1):       # step temp press pe ke as printed (%.8g or better)
        rows_ok = rows_ok and all(abs(u - v) <= 2e-7 * max(abs(v), 1.0) for u, v in zip(a, b))
    err = dict(dx=float(np.abs(dx).max()), dv=float(np.abs(vn - v1).max()), rows=0 if rows_ok else 1,
               builds=out.split("Neighbor list builds = ")[1].split()[0])
    return err, dict(dx=1e-8, dv=1e-7, rows=1)


def line_dd(spec, err):
    return (f"{spec['style']} ranks {spec['ranks']} rep {spec['rep']} T {spec['temp']} drift {spec['drift']} steps {spec['steps']} "
            f"seed {spec['seed']} {spec['extra']} dx {err['dx']:.2e} dv {err['dv']:.2e} builds {err['builds']}")


# ------------------------------------------------------------------------------------------------------- hostmode_walk
# HOST-MODE walks (the plain plugin path: atoms uploaded once, then positions every step, the library deciding by itself
# when its own lists and pruned rows are stale): random cells, then 40 steps of a random walk (every atom a little, one
# atom a lot, some steps nobody) inside the host's skin, forces against the oracle at EVERY step.
def draw_hostmode_walk(rng):
    style = rng.choice(["rebomos", "aeam"]); sd = rng.randrange(1, 10**6)
    images = rng.random() < 0.5     # one periodic rank: the library keeps the images itself, the host's ghost positions are poison
    if style == "rebomos":
        fac, amp, rep = rng.uniform(0.95, 1.12), rng.uniform(0.0, 0.15), rng.choice([None, (2, 1, 1), (1, 2, 1)])
        spec = dict(fac=fac, amp=amp, rep=rep, skin=2.0, n=_rebo_n(rep), env=_inner(rng, [0.3, 0.6]))
    else:
        cells, frac, amp = rng.choice([4, 5, 6]), rng.choice([0.0075, 0.08, 0.3]), rng.uniform(0.0, 0.15)
        spec = dict(cells=cells, frac=frac, amp=amp, skin=1.0, n=4 * cells ** 3, env={})
    walk = []
    for _ in range(40):
        mode = rng.choice(["all", "all", "one", "none", "few"])
        arg = rng.choice([0.002, 0.01, 0.03]) if mode == "all" else (rng.randrange(spec["n"]) if mode == "one" else None)
        walk.append((mode, arg))
    spec.update(style=style, seed=sd, images=images, walk=walk, id=f"{style}-n{spec['n']}-images{int(images)}")
    return spec


def run_hostmode_walk(spec):
    import fixture_cases as FC
    import oracle_bindings as ob
    from lammps_plugins_amd.host import capi
    R = _res()
    style, sd, images, skin = spec["style"], spec["seed"], spec["images"], spec["skin"]
    nr = np.random.default_rng(sd)
    if style == "rebomos":
        s = FC._rebomos(spec["fac"], spec["amp"], sd, spec["rep"])
        eng = FC.engine(style, s, R["orc"], P=R["P"])
    else:
        s = FC._aeam_cell(spec["cells"], spec["frac"], spec["amp"], sd)
        eng = FC.engine(style, s, R["orc"], T=R["T"])
    assert s.n == spec["n"]
    worst, at = 0.0, ""
    ctx = capi.Context(0)
    try:
        if style == "rebomos":
            ctx.rebomos_set_params(R["rp"])
        else:
            ctx.aeam_set_tables(R["tabs"]); ctx.aeam_device_lists(True)
        if images: ctx.set_box_host(s.box)
        ctx.set_atoms_host(eng.nlocal, eng.all_positions(s.x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1] if style == "rebomos" else None)
        ctx.set_skin(skin)
        x = s.x.copy(); x0 = x.copy(); n = s.n; owner = eng.owner
        for step, (mode, arg) in enumerate(spec["walk"]):
            dxs = np.zeros((n, 3))
            if mode == "all": dxs = nr.normal(0.0, arg, (n, 3))
            elif mode == "one": dxs[arg] = nr.normal(0.0, 0.15, 3)
            elif mode == "few": dxs[nr.integers(0, n, 5)] = nr.normal(0.0, 0.08, (5, 3))
            xn = x + dxs
            # stay inside the host's list: no atom further than 0.45 skin from where the lists were built
            far = np.linalg.norm(xn - x0, axis=1) > 0.45 * skin
            xn[far] = x[far]
            x = xn
            xa = eng.all_positions(x)
            if images:
                xa = xa.copy(); xa[eng.nlocal:] = np.nan
            ctx.set_positions_host(xa)
            o = eng.compute(x, eflag=1, vflag=0)
            if style == "rebomos":
                f = ctx.rebomos_compute_host(eng.nlocal, eflag=0 if step % 3 else 1, vflag=0)["f"]
            elif images:   # fp and the images' share of the three-body forces stay on the device
                ctx.aeam_density_host(eng.nlocal, eflag=0, keep_fp=True)
                f = ctx.aeam_force_host(len(xa), eng.nlocal, None, eflag=0, vflag=0)["f"][:eng.nlocal]
            else:
                d = ctx.aeam_density_host(eng.nlocal, eflag=0)
                r = ctx.aeam_force_host(len(xa), eng.nlocal, np.concatenate([d["fp"], d["fp"][owner]]), eflag=0, vflag=0)
                f = ob.fold_ghost_forces(r["f"], owner, eng.nlocal)
            err = float(np.abs(f - o["f_owned"]).max()) / max(1.0, float(np.abs(o["f_owned"]).max()))
            if err > worst: worst, at = err, f"worst at step {step} ({mode})"
    finally:
        ctx.close()
    return dict(dF=worst, at=at), dict(dF=1e-9)


def line_hostmode_walk(spec, err):
    return (f"{spec['style']} n {spec['n']} images {spec['images']} seed {spec['seed']} inner {spec['env'].get('MDP_INNER_SKIN')} "
            f"dF {err['dF']:.1e} {err['at']}")


# ---------------------------------------------------------------------------------------------------------------- hnve
# What `fix nve/mdp` does on one rank in its default mode (mdp_hnve_initial / compute with f == NULL / mdp_hnve_final,
# the images kept by the library, the device's displacement check read one step late and a HOST reneighboring when it
# fires): random MoS2 cells up to 3 000 K, a projectile in some, against velocity Verlet around the ORACLE.
def draw_hnve(rng):
    sd = rng.randrange(1, 10**6)
    rep = rng.choice([None, (2, 1, 1), (1, 2, 1)]); temp = rng.choice([300, 1200, 3000]); skin = rng.choice([1.0, 2.0])
    n = _rebo_n(rep)
    shot = rng.random() < 0.4
    shot_atom = rng.randrange(n) if shot else None
    return dict(seed=sd, rep=rep, temp=temp, skin=skin, n=n, shot=shot, shot_atom=shot_atom, nsteps=90, env=_inner(rng, [0.3, 0.5]),
                id=f"n{n}-T{temp}-skin{skin}-shot{int(shot)}")


def run_hnve(spec):
    import mdref
    import oracle_bindings as ob
    import test_gpu_trajectory as TT
    from lammps_plugins_amd.host import capi
    R = _res(); orc, P = R["orc"], R["P"]
    sd, rep, skin, nsteps = spec["seed"], spec["rep"], spec["skin"], spec["nsteps"]
    s = S.rebomos_bulk_cell() if rep is None else S.replicate(S.rebomos_bulk_cell(), rep)
    v0 = S.gaussian_velocities(s, float(spec["temp"]), seed=sd)
    if spec["shot"]: v0[spec["shot_atom"]] += np.array([20.0, -22.0, 18.0])
    host = TT._host_run(lambda sy: mdref.RebomosCPU(orc, P, sy, skin=skin), s, v0, nsteps, nsteps, skin, rebuild_every=10)
    x = S.wrap(s.box, s.x); v = v0.copy(); rebuilds = 0
    c = capi.Context(0)

    def upload(x, v):
        eng = mdref.RebomosCPU(None, P, S.System(s.box, x.copy(), s.type, s.tag, s.mass), skin=skin)   # ghosts only
        c.set_box_host(s.box)
        c.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
        c.set_skin(skin)
        c.hnve_upload_v(v)
    try:
        c.rebomos_set_params(ob.product_rebomos_params(P))
        c.hnve_setup(0.001, S.FTM2V, s.mass)
        upload(x, v)
        c.rebomos_compute_host(s.n, eflag=0, vflag=0)
        late_any = False
        for step in range(nsteps):
            moved, late = c.hnve_initial()
            late_any |= late
            if moved:   # the host reneighbors: what Verlet::run does when Neighbor::decide() says so
                got = c.hnve_download(s.n, want=("x", "v"))
                upload(S.wrap(s.box, got["x"]), got["v"]); rebuilds += 1
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
            c.hnve_final()
        got = c.hnve_download(s.n, want=("x", "v"))
    finally:
        c.close()
    xh = host[nsteps][0]
    dx = got["x"] - xh; dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
    hot = spec["temp"] >= 3000 or spec["shot"]
    return dict(dx=float(np.abs(dx).max()), late=int(late_any), rebuilds=rebuilds), dict(dx=1e-6 if hot else 1e-8, late=1)


def line_hnve(spec, err):
    return (f"n {spec['n']} T {spec['temp']} skin {spec['skin']} shot {spec['shot']} seed {spec['seed']} inner {spec['env'].get('MDP_INNER_SKIN')} "
            f"dx {err['dx']:.1e} host rebuilds {err['rebuilds']} late {bool(err['late'])}")


# ------------------------------------------------------------------------------------------------------------- minilmp
# The plugins on N ranks of the mini-host: the thermo rows of `minilmp -np N` -- in host mode and under `fix nve/mdp` on
# the library's bricks; on one rank: the fix in its default mode and with `bricks yes` -- must be the rows of the
# one-rank run with the host's own `fix nve` (printed digits: rel 5e-7).
def draw_minilmp(rng):
    np_ = rng.choice([1, 1, 2, 3, 4, 6, 8])
    if rng.random() < 0.5:
        rep = rng.choice(["2 2 1", "2 2 2", "3 2 1", "1 2 2", "3 3 1"]); T = rng.choice([300, 900, 1500, 4000]); skin = rng.choice([0.4, 0.8, 2.0])
        steps = rng.choice([60, 120, 200]); sd = rng.randrange(1, 10**7)
        spec = dict(style="rebomos", rep=rep, T=T, skin=skin, steps=steps, seed=sd,
                    desc=f"rebomos rep {rep} T {T} skin {skin} steps {steps} seed {sd}")
    else:
        n = rng.choice([8, 10, 12, 14]); T = rng.choice([300, 863, 1400, 3000]); steps = rng.choice([60, 100, 160]); sd = rng.randrange(1, 10**7)
        frac = rng.choice([0.0075, 0.03, 0.08])
        spec = dict(style="aeam", cells=n, frac=frac, T=T, steps=steps, seed=sd,
                    desc=f"aeam cells {n} frac {frac} T {T} steps {steps} seed {sd}")
    spec.update(np=np_, env={}, id=f"{spec['style']}-np{np_}-T{spec['T']}-steps{spec['steps']}")
    return spec


def minilmp_input(spec):
    if spec["style"] == "rebomos":
        text = open(os.path.join(PKG, "examples", "in.rebomos-bulk.mi355x")).read()
        text = text.replace("create_atoms 2 box basis 1 1 basis 2 1 basis 3 2 basis 4 2 basis 5 2 basis 6 2",
                            "create_atoms 2 box basis 1 1 basis 2 1 basis 3 2 basis 4 2 basis 5 2 basis 6 2\nreplicate " + spec["rep"])
        text = text.replace("thermo 10", f"velocity all create {spec['T']}.0 {spec['seed']}\nneighbor {spec['skin']} bin\nthermo {spec['steps'] // 4}").replace("run 20", f"run {spec['steps']}")
    else:
        n = spec["cells"]
        text = open(os.path.join(PKG, "examples", "in.aeam-alsi.mi355x")).read()
        text = text.replace("region MeSi block 0 20 0 20 0 20", f"region MeSi block 0 {n} 0 {n} 0 {n}").replace("type/fraction 2 0.0075 7683797", f"type/fraction 2 {spec['frac']} {spec['seed']}")
        text = text.replace("velocity all create 863.0 1082337", f"velocity all create {spec['T']}.0 {spec['seed']}").replace("thermo 100", f"thermo {spec['steps'] // 4}").replace("run 400", f"run {spec['steps']}")
    assert "fix integrate all nve" in text
    return text


def _rows_equal(a, b):
    if len(a) != len(b) or not a: return False
    for r, q in zip(a, b):
        for u, v in zip(r, q):
            if abs(u - v) > 5e-7 * max(abs(v), 1.0) + 1e-5: return False
    return True


def run_minilmp(spec):
    from test_plugin_boundary import _run, _thermo_rows
    from lammps_plugins_amd.host import capi
    env = dict(MDP_RCCL_LIBRARY=capi.FAKE_RCCL, MDP_FAKE_RCCL_TIMEOUT_S="60", MDP_FIX_STATS="1")
    text, np_ = minilmp_input(spec), spec["np"]
    rc0, out0, _ = _run(text)
    if np_ == 1:   # one rank: the fix in its default mode (the host reneighbors) and with one brick of the library's
        rc1, out1, err1 = _run(text.replace("fix integrate all nve", "fix integrate all nve/mdp"), env=env)
        rc2, out2, err2 = _run(text.replace("fix integrate all nve", "fix integrate all nve/mdp bricks yes"), env=env)
    else:
        rc1, out1, err1 = _run(text, np=np_)
        rc2, out2, err2 = _run(text.replace("fix integrate all nve", "fix integrate all nve/mdp"), np=np_, env=env)
    r0, r1, r2 = _thermo_rows(out0), _thermo_rows(out1), _thermo_rows(out2)
    err = dict(rc=0 if rc0 == rc1 == rc2 == 0 else 1, rows_host=0 if _rows_equal(r1, r0) else 1, rows_fix=0 if _rows_equal(r2, r0) else 1,
               nrows=len(r0), host_builds=out0.split("Neighbor list builds = ")[-1].split()[0],
               reneighborings=out2.split("reneighborings on the device")[0].split()[-1] if "reneighborings on the device" in out2 else "?",
               rcs=f"{rc0} {rc1} {rc2}", stderr=f"{err1[-200:]} {err2[-200:]}")
    return err, dict(rc=1, rows_host=1, rows_fix=1)


def line_minilmp(spec, err):
    ok = not (err["rc"] or err["rows_host"] or err["rows_fix"])
    return (f"np {spec['np']} {spec['desc']} rows {err['nrows']} host builds {err['host_builds']} device reneighborings {err['reneighborings']}"
            + ("" if ok else f" rc {err['rcs']} {err['stderr']}"))


# ---------------------------------------------------------------------------------------------------------- trajectory
# Device-resident trajectories against the same trajectories driven on the host with ORACLE forces: small MoS2 cells and
# Al-Si alloys (half of them sheared), up to 4 000 K, a fast projectile in some, 120 steps with the device's own deferred
# checks, row prunings, list rebuilds and reneighborings.  Positions 1e-8 A (hot cases 1e-6: the trajectories are
# chaotic), energy 1e-9 eV per atom, no late pruning.
def draw_trajectory(rng):
    style = rng.choice(["rebomos", "aeam"]); sd = rng.randrange(1, 10**6)
    if style == "rebomos":
        rep = rng.choice([None, (2, 1, 1), (1, 2, 1)]); temp = rng.choice([300, 1500, 4000])
        spec = dict(rep=rep, temp=temp, skin=2.0, n=_rebo_n(rep), env=_inner(rng, [0.3, 0.5, 1.0]), tilt=None)
    else:
        n = rng.choice([4, 5, 6]); temp = rng.choice([300, 863, 2500]); frac = rng.choice([0.0, 0.03, 0.2])
        spec = dict(cells=n, temp=temp, frac=frac, skin=1.0, n=4 * n ** 3, env={}, tilt=None)
        if rng.random() < 0.5:   # a sheared (triclinic) box
            L = 4.045 * n
            spec["tilt"] = [rng.uniform(-0.06, 0.06) * L for _ in range(3)]
    shot = rng.random() < 0.4
    spec["shot"] = (rng.randrange(spec["n"]), rng.choice([-1, 1])) if shot else None
    spec.update(style=style, seed=sd, nsteps=120, id=f"{style}-n{spec['n']}-T{spec['temp']}-shot{int(shot)}")
    return spec


def run_trajectory(spec):
    import mdref
    import test_gpu_trajectory as TT
    from lammps_plugins_amd.host import capi
    R = _res(); orc, P, T, rp, af, tabs = R["orc"], R["P"], R["T"], R["rp"], R["af"], R["tabs"]
    style, sd, skin, nsteps = spec["style"], spec["seed"], spec["skin"], spec["nsteps"]
    if style == "rebomos":
        s = S.rebomos_bulk_cell() if spec["rep"] is None else S.replicate(S.rebomos_bulk_cell(), spec["rep"])
    else:
        s = S.fcc_cell(4.045, spec["cells"], frac_type2=spec["frac"], seed=sd); s.mass[1:3] = af.mass[:2]
        if spec["tilt"] is not None:
            nb = S.Box(s.box.lo.copy(), s.box.prd.copy(), np.array(spec["tilt"]))
            s = S.System(nb, nb.lamda2x(s.box.x2lamda(s.x)), s.type, s.tag, s.mass)
    v0 = S.gaussian_velocities(s, float(spec["temp"]), seed=sd + 1)
    if spec["shot"]: v0[spec["shot"][0]] += np.array([spec["shot"][1] * 22.0, 20.0, 18.0])   # a projectile at ~35 A/ps
    ctx = capi.Context(0)
    try:
        if style == "rebomos":
            host = TT._host_run(lambda sy: mdref.RebomosCPU(orc, P, sy, skin=skin), s, v0, nsteps, 30, skin, rebuild_every=10)
            ctx.rebomos_set_params(rp)
            dev, d = TT._device_run(ctx, capi.STYLE_REBOMOS, s, v0, nsteps, 30, skin, 3.0 * rp.rcmax[0][0] + skin, [0, 0, 1])
        else:
            host = TT._host_run(lambda sy: mdref.AeamCPU(orc, T, sy, skin=skin), s, v0, nsteps, 30, skin, rebuild_every=5)
            ctx.aeam_set_tables(tabs)
            dev, d = TT._device_run(ctx, capi.STYLE_AEAM, s, v0, nsteps, 30, skin, float(af.cut_table(tabs).max()) + skin, None)
        pr = ctx.md_prune_stats()
    finally:
        ctx.close()
    hot = spec["temp"] >= 2500 or spec["shot"] is not None
    xtol, etol = (1e-6, 1e-8) if hot else (1e-8, 1e-9)
    wx, we = TT._compare(s, host, dev, xtol=np.inf, etol=np.inf)   # (worst values; the limits are applied below)
    return (dict(dx=wx, dE_atom=we, late=pr["late"], prunings=pr["prunings"], builds=d.builds, tilt=np.round(s.box.tilt, 1).tolist()),
            dict(dx=xtol, dE_atom=etol, late=1))


def line_trajectory(spec, err):
    return (f"{spec['style']} n {spec['n']} tilt {err.get('tilt', '?')} T {spec['temp']} shot {spec['shot'] is not None} seed {spec['seed']} "
            f"inner {spec['env'].get('MDP_INNER_SKIN')} dx {err['dx']:.1e} dE/atom {err['dE_atom']:.1e} prunings {err['prunings']} "
            f"late {err['late']} builds {err['builds']}")


# --------------------------------------------------------------------------------------------------------------- block
# Parity at scale: systems of 70 000 - 390 000 atoms (MoS2 replicas scaled by 0.97 - 1.12 with jitter, or Al-Si alloys
# with 0 - 20 % Si) run device-resident for 20 - 60 steps from 300 - 3 000 K (lists rebuilt and rows pruned on the
# device's own triggers), then the forces of ~400-atom blocks at the box corners, the brick seams, the last tile and
# random places against the ORACLE's for the same atoms (tests/blockcheck.py), 1e-9 eV/A; no late pruning.
def draw_block(rng):
    style = rng.choice(["rebomos", "aeam"]); sd = rng.randrange(1, 10**6); steps = rng.choice([20, 40, 60])
    if style == "rebomos":
        rep = rng.choice([(6, 5, 8), (7, 6, 8), (8, 7, 9), (10, 9, 10), (12, 10, 10)])
        fac, amp, temp = rng.choice([0.97, 1.0, 1.0, 1.05, 1.12]), rng.choice([0.0, 0.05, 0.15]), rng.choice([300, 1000, 3000])
        spec = dict(rep=rep, fac=fac, amp=amp, temp=temp, n=_rebo_n(rep), env=_inner(rng, [0.4, 0.6, 1.0]),
                    desc=f"rep {rep} fac {fac} amp {amp}")
    else:
        n = rng.choice([28, 32, 36, 40, 46]); frac, temp = rng.choice([0.0, 0.0075, 0.08, 0.2]), rng.choice([300, 863, 2500])
        spec = dict(cells=n, frac=frac, temp=temp, n=4 * n ** 3, env={}, desc=f"cells {n} frac {frac}")
    spec.update(style=style, seed=sd, steps=steps, id=f"{style}-n{spec['n']}-T{spec['temp']}-steps{steps}")
    return spec


def run_block(spec):
    import blockcheck
    import mdref
    from lammps_plugins_amd.host import capi, resident
    R = _res(); orc, P, T, rp, af, tabs = R["orc"], R["P"], R["T"], R["rp"], R["af"], R["tabs"]
    sd = spec["seed"]
    ctx = capi.Context(0)
    try:
        if spec["style"] == "rebomos":
            s = S.replicate(S.rebomos_bulk_cell(), spec["rep"])
            if spec["fac"] != 1.0: s = S.scale(s, spec["fac"])
            if spec["amp"]: s = S.jitter(s, spec["amp"], seed=sd)
            ctx.rebomos_set_params(rp)
            skin, cutghost, map_, st = 2.0, 3.0 * rp.rcmax[0][0] + 2.0, [0, 0, 1], capi.STYLE_REBOMOS
            factory, shell, margin = (lambda cs: mdref.RebomosCPU(orc, P, cs)), 11.0, 16.0
        else:
            s = S.fcc_cell(4.045, spec["cells"], frac_type2=spec["frac"], seed=sd); s.mass[1:3] = af.mass[:2]
            ctx.aeam_set_tables(tabs)
            skin, cutghost, map_, st = 1.0, float(af.cut_table(tabs).max()) + 1.0, None, capi.STYLE_AEAM
            factory, shell, margin = (lambda cs: mdref.AeamCPU(orc, T, cs)), 13.5, 10.0
        v0 = S.gaussian_velocities(s, float(spec["temp"]), seed=sd + 1)
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.compute(0, 0)
        for _ in range(spec["steps"]): d.step(0, 0, rebuild="auto")
        pr = ctx.md_prune_stats()
        got = ctx.md_download(d.nlocal, want=("x", "f"))
        tags, types = d.tags_local, ctx.md_download_int("type", d.nlocal)
        builds = d.builds
    finally:
        ctx.close()
    pts = blockcheck.seeds(s.box, got["x"], n_random=3, seed=sd)
    worst, rows = blockcheck.check_blocks(s.box, got["x"], got["f"], types, tags, s.mass, pts, factory, n_interior=400,
                                          shell=shell, margin=margin, tol=1e-9)
    return dict(dF=worst, late=pr["late"], blocks=len(rows), prunings=pr["prunings"], builds=builds), dict(dF=1e-9, late=1)


def line_block(spec, err):
    return (f"{spec['style']} n {spec['n']} {spec['desc']} T {spec['temp']} steps {spec['steps']} seed {spec['seed']} "
            f"inner {spec['env'].get('MDP_INNER_SKIN')} worst dF {err['dF']:.1e} over {err['blocks']} blocks "
            f"prunings {err['prunings']} late {err['late']} builds {err['builds']}")


# --------------------------------------------------------------------------------------------------------------- fire
# The FIRE minimiser under random `min_modify` settings: every setting from a short list that holds the default, each
# value that makes a branch degenerate (delaystep 0, dtgrow 1, dtshrink 1, alphashrink 1, tmax 1, tmin 1) and one other;
# halfstepback and initialdelay on or off; starting time steps of 1, 2 and 4 fs; the small cells of both styles with more
# jitter and strain.  80 device iterations REPLAYED one at a time (tests/firerig.py): decisions, dt and alpha exact; dtv,
# s1, s2, x and v to 1e-13; and the forces of every iteration against the oracle's at the downloaded positions (1e-9
# eV/A), so a pair the advance kernel's displacement prediction misses shows in the iteration it happens.
# The ceiling of the time step (tmax dt) is kept at or below 10 fs: beyond it fireref with oracle forces itself blows up.
# Measured on an MI355X (seed 4, 16 cases; 200 more at seed 11): x 3.6e-15 A, v 3.5e-15, dtv / s1 / s2
# 5.4e-16, forces 5.4e-13 eV/A over all cases; the device sits orders below the limits, which stay where they are.
FIRE_MODIFY = dict(dmax=(0.1, 0.02, 0.005), tmax=(10.0, 2.0, 1.0), tmin=(0.02, 0.5, 1.0), delaystep=(20, 0, 3, 8),
                   dtgrow=(1.1, 1.0, 1.3), dtshrink=(0.5, 0.9, 1.0), alpha0=(0.25, 0.05, 0.6), alphashrink=(0.99, 0.9, 1.0),
                   halfstepback=(True, False), initialdelay=(True, False))
FIRE_ITERATIONS = 80
FIRE_SKIPPED = {}     # (id, seed) -> iterations not replayed, of the cases run in this process (a record, not a limit)


def draw_fire(rng):
    style = rng.choice(["rebomos", "aeam"])
    jitter, scale, sd = rng.choice([0.05, 0.15, 0.3]), rng.choice([1.0, 1.06]), rng.randrange(1, 10**6)
    dt = rng.choice([0.001, 0.002, 0.004])
    modify = {k: rng.choice(v) for k, v in FIRE_MODIFY.items()}
    if modify["tmax"] * dt > 0.0101:
        # The ceiling of the time step stays at or below 10 fs, what the defaults give at 1 fs.  Beyond it FIRE is no
        # minimiser for these potentials: with oracle forces fireref itself blows up (atoms fly hundreds of A at a
        # ceiling of 20 or 40 fs), and forces of 1e5 eV/A cannot be held to 1e-9.  The other values of tmax stay.
        modify["tmax"] = 2.0
    odd = [f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in modify.items() if v != FIRE_MODIFY[k][0]]
    return dict(style=style, jitter=jitter, scale=scale, seed=sd, dt=dt, modify=modify, niter=FIRE_ITERATIONS, env={},
                id=f"{style}-dt{dt}-" + ("-".join(odd) or "defaults"))


def trace_fire(spec):
    """no GPU: fireref.minimize with ORACLE forces over the case's iterations; one row per iteration, for the corner
    test of tests/test_net_draws.py: dict(iter, mixed, dt_before, dt, dtv, moved: the farthest an atom went so far)"""
    import firerig
    import fireref
    s = firerig.cell(spec["style"], jitter=spec["jitter"], scale=spec["scale"], seed=spec["seed"])
    orc_f = firerig.Forces(spec["style"], _res()["orc"], s)
    x0 = S.wrap(s.box, s.x)
    rows, last = [], dict(dt=spec["dt"], moved=0.0)

    def fe(x):
        o = orc_f(x, eflag=1)
        return o["f_owned"], o["eng"]

    def record(fire, _):
        last["moved"] = max(last["moved"], float(np.sqrt(((fire.x - x0) ** 2).sum(axis=1)).max()))
        rows.append(dict(iter=fire.iter, mixed=fire.mixed, dt_before=last["dt"], dt=fire.dt, dtv=fire.dtv, moved=last["moved"]))
        last["dt"] = fire.dt
    fireref.minimize(fe, x0, s.mass[s.type], spec["dt"], S.FTM2V, 0.0, 0.0, spec["niter"], 10 ** 9, record=record, **spec["modify"])
    return rows


def run_fire(spec):
    import firerig
    s = firerig.cell(spec["style"], jitter=spec["jitter"], scale=spec["scale"], seed=spec["seed"])
    rig = firerig.Rig(spec["style"], s, _res()["orc"], dt=spec["dt"])
    try:
        rig.ctx.fire_setup(0.0, 0.0, firerig.BIG, firerig.BIG, **spec["modify"])
        r = firerig.replay(rig, spec["niter"], modify=spec["modify"], forces=True)
        st = rig.ctx.fire_state()
    finally:
        rig.close()
    err = dict(exact=len(r["exact"]), ctl=r["ctl"], x=r["x"], v=r["v"], f=r["f"], skipped=r["skipped"], late=st["late"],
               first_mismatch=r["exact"][:1], negatives=len(r["negatives"]), grown=r["grown"], limited=r["limited"], ceiling=r["ceiling"],
               moved=r["moved"], reneighbors=st["reneighbors"])
    FIRE_SKIPPED[spec["id"], spec["seed"]] = r["skipped"]
    # (a case may skip one iteration in its 80; that the suite's cases together skip at most 1 in 100 is asserted over
    # the whole suite by tests/test_gpu_fire_mdp.py)
    return err, dict(exact=1, ctl=1e-13, x=1e-13, v=1e-13, f=1e-9, skipped=2, late=1)


def line_fire(spec, err):
    return (f"{spec['id']} jitter {spec['jitter']} scale {spec['scale']} seed {spec['seed']} x {err['x']:.1e} v {err['v']:.1e} "
            f"dtv/s1/s2 {err['ctl']:.1e} dF {err['f']:.1e} P<=0 {err['negatives']} grown {err['grown']} at dtmax {err['ceiling']} "
            f"dmax-limited {err['limited']} skipped {err['skipped']} moved {err['moved']:.2f} A reneighbourings {err['reneighbors']} "
            f"late {err['late']}" + (f" MISMATCH {err['first_mismatch']}" if err["exact"] else ""))


# ----------------------------------------------------------------------------------------------------------- langevin
# The Langevin thermostat on every path that reaches the integrate kernel -- resident with the device's own check
# ("resident"), resident through mdp_md_initial_integrate / mdp_md_final_initial_integrate with forced reneighbourings
# ("resident-plain": the CHECK = false instantiations), host-linked (mdp_hnve_*, host reneighbourings) and 2 - 8 bricks
# on the thread transport with a drift that makes atoms change owner -- against velocity Verlet + tests/langevinref.py
# around the ORACLE (refloops.host_lgv): first steps below, across and above 2^32 (the second counter word
# of the noise), time steps of 0.5 - 2 fs, targets that ramp up, down to 0 K or stay at 0 K, scale ratios, zero, tally,
# thermo reads that complete a deferred final half or follow one that ran on its own, sizes whose last 256-atom block
# varies, sheared alloy boxes.  Limits (from a CPU experiment with the reference): positions 1e-9 A,
# velocities 2e-8 A/ps, tally 1e-8 eV; bricks against the one-rank device run 1e-8 A, 1e-7 A/ps (the dd net's).
# Measured on an MI355X (seed 42, 14 cases; 200 more at seed 11): 3.0e-13 A, 5.5e-12 A/ps, 1.3e-12 eV; bricks 2.1e-14 A,
# 1.2e-12 A/ps from one rank.  Four to five orders below the limits, as the NVE nets are; the limits are the reference's, not the device's.
LGV_PATHS = ("resident", "resident-plain", "hostlinked", "bricks")
LGV_FIRST = (0, 1000, 2 ** 32 - 30, 2 ** 32 + 7, 5 * 2 ** 32)
LGV_TEMPS = ((300.0, 300.0), (300.0, 900.0), (900.0, 2000.0), (3000.0, 0.0), (0.0, 0.0))
LGV_RATIOS = {"none": None, "all": {1: 2.0, 2: 0.5}, "one": {2: 0.5}}
LGV_SEED = 48271
LGV_REBUILD = {"rebomos": 25, "aeam": 10}       # steps between the reference's list builds (skins 2.0 and 1.0 A)


def draw_langevin(rng):
    style = rng.choice(["rebomos", "aeam"])
    path = rng.choice(LGV_PATHS)
    first, nsteps = rng.choice(LGV_FIRST), rng.choice([40, 60, 100])
    dt, damp = rng.choice([0.0005, 0.001, 0.002]), rng.choice([0.01, 0.05, 0.1])
    t0, t1 = rng.choice(LGV_TEMPS)
    ratio = rng.choice(["none", "all", "one"])
    zero, tally = rng.random() < 0.5, rng.random() < 0.5
    if style == "rebomos":
        size = rng.choice([(1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 1)])
        spec = dict(size=size, n=_rebo_n(size), frac=None, tilt=None, skin=2.0)
    else:
        size, frac = rng.choice([4, 5, 6, 7]), rng.choice([0.0, 0.03])
        spec = dict(size=size, n=4 * size ** 3, frac=frac, tilt=None, skin=1.0)
        if rng.random() < 0.5:   # a sheared (triclinic) box
            spec["tilt"] = [rng.uniform(-0.06, 0.06) * 4.045 * size for _ in range(3)]
    # thermo reads at random steps, the last step among them; True: the read finds the step's final half deferred and
    # completes it, False: the final half ran on its own (f + f_L written back) before the read
    reads = [(st, rng.random() < 0.5) for st in sorted(rng.sample(range(1, nsteps), rng.randint(1, 4))) + [nsteps]]
    ranks, renb = rng.choice([2, 3, 4, 8]), rng.choice([3, 5, 8])
    drift = [0, 0, 0]
    while not any(drift):
        drift = [rng.choice([-60, -30, 0, 25, 40, 70]) for _ in range(3)]
    if path == "bricks":
        zero = tally = False     # (they sum over all atoms every step: one rank only)
    else:
        ranks, drift = 1, [0, 0, 0]
    spec.update(style=style, path=path, first=first, nsteps=nsteps, dt=dt, damp=damp, t0=t0, t1=t1, ratio=ratio, zero=zero,
                tally=tally, reads=reads, ranks=ranks, drift=drift, renb=renb, seed=rng.randrange(1, 10**6), env={},
                id=f"{style}-{path}{ranks if ranks > 1 else ''}-n{spec['n']}-first{first}-dt{dt}-T{t0:.0f}-{t1:.0f}")
    return spec


def _lgv_system(spec):
    """the system, its start velocities (max(Tstart, 300) K, plus the drift) and the steps between forced list builds:
    the drawn interval, shortened until an atom at the drift plus five thermal sigmas of the hottest target stays
    inside 0.3 skin"""
    af = _res()["af"]
    if spec["style"] == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), spec["size"])
    else:
        s = S.fcc_cell(4.045, spec["size"], frac_type2=spec["frac"], seed=spec["seed"]); s.mass[1:3] = af.mass[:2]
        if spec["tilt"] is not None:
            nb = S.Box(s.box.lo.copy(), s.box.prd.copy(), np.array(spec["tilt"]))
            s = S.System(nb, nb.lamda2x(s.box.x2lamda(s.x)), s.type, s.tag, s.mass)
    assert s.n == spec["n"]
    v0 = S.gaussian_velocities(s, max(spec["t0"], 300.0), seed=spec["seed"] + 1) + np.array(spec["drift"], dtype=float)
    hot = max(spec["t0"], spec["t1"], 300.0)
    vcap = float(np.sqrt((v0 ** 2).sum(axis=1)).max()) + 5.0 * np.sqrt(S.BOLTZ * hot / (float(s.mass[1:3].min()) * S.MVV2E))
    safe = max(1, int(0.3 * spec["skin"] / (vcap * spec["dt"])))
    return s, v0, safe


def _lgv_context(style):
    from lammps_plugins_amd.host import capi
    R = _res()
    ctx = capi.Context(0)
    if style == "rebomos":
        ctx.rebomos_set_params(R["rp"])
        return ctx, capi.STYLE_REBOMOS, 3.0 * R["rp"].rcmax[0][0] + 2.0, [0, 0, 1]
    ctx.aeam_set_tables(R["tabs"])
    return ctx, capi.STYLE_AEAM, float(R["af"].cut_table(R["tabs"]).max()) + 1.0, None


def _lgv_device(spec, s, v0, world, rebuild_every):
    """the case on `world` resident bricks (threads beyond one).  rebuild_every None: the device's own check
    (rebuild="auto"); a number: the integrate calls without the check, reneighbourings forced every so many steps.
    Returns {step: (x, v by tag, tally, the rank that holds each tag)}, the atoms that changed owner, whether every tag
    was held exactly once at every read, list builds, late checks."""
    from lammps_plugins_amd.host import resident
    reads = dict(spec["reads"])

    def rank_fn(r, make_tr):
        ctx, st, cutghost, map_ = _lgv_context(spec["style"])
        try:
            d = resident.DeviceDomain(ctx, st, s, cutghost, spec["skin"], map_, v0=v0, dt=spec["dt"],
                                      transport=make_tr(ctx) if world > 1 else None)
            d.langevin(spec["t0"], spec["t1"], spec["damp"], LGV_SEED, ratio=LGV_RATIOS[spec["ratio"]], zero=spec["zero"],
                       tally=spec["tally"], first=spec["first"], last=spec["first"] + spec["nsteps"])
            d.compute(1, 0)
            out, left = {}, 0
            for step in range(1, spec["nsteps"] + 1):
                ev = step in reads
                rb = "auto" if rebuild_every is None else step % rebuild_every == 0
                d.step(1 if ev else 0, 0, rebuild=rb, defer_final=reads.get(step, True))
                if rb is True:
                    left += ctx.dd_info()["left_last"]
                if ev:   # through the library, not DeviceDomain.flush: a deferred final half is completed by the read itself
                    e = ctx.langevin_tally()
                    got = ctx.md_download(d.nlocal, want=("x", "v"))
                    out[step] = (d.tags_local.copy(), got["x"], got["v"], e)
            return dict(out=out, left=left, builds=d.builds, late=d.dangerous)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    dev, once = {}, True
    for step in reads:
        x, v, seen, owner = np.zeros((s.n, 3)), np.zeros((s.n, 3)), np.zeros(s.n, dtype=int), np.zeros(s.n, dtype=int)
        for k, r in enumerate(res):
            tags, xr, vr, _ = r["out"][step]
            x[tags - 1], v[tags - 1], owner[tags - 1] = xr, vr, k
            seen[tags - 1] += 1
        once = once and bool(np.all(seen == 1))
        dev[step] = (x, v, res[0]["out"][step][3], owner)
    return dev, sum(r["left"] for r in res), once, res[0]["builds"], sum(r["late"] for r in res)


def _lgv_hostlinked(spec, s, v0, rebuild_every):
    """mdp_hnve_* with the thermostat: the images kept by the library, host reneighbourings (download, wrap, new atoms,
    mdp_hnve_upload_v) every rebuild_every steps and earlier whenever mdp_hnve_initial reports `moved`.  REBO-MoS, and the
    alloy on the library's own lists (mdp_aeam_device_lists): fp and the forces stay on the device, as under the plugin's
    fix nve/mdp."""
    import ctypes as C
    import oracle_bindings as ob
    from lammps_plugins_amd.host import capi
    R = _res()
    style, n, skin = spec["style"], s.n, spec["skin"]
    cut = (R["P"].cut3rebo if style == "rebomos" else float(R["af"].cut_table(R["tabs"]).max())) + skin
    c = capi.Context(0)

    def upload(x, v):
        xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), s.type, s.tag, s.mass), cut)
        c.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=[0, 0, 1] if style == "rebomos" else None)
        c.set_skin(skin)
        c.hnve_upload_v(v)

    def compute():   # f == NULL: the forces' only reader is the device's integrator
        if style == "rebomos":
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
        else:
            eng, vir = C.c_double(0.0), np.zeros(6)
            c._ck(c.L.mdp_aeam_density_host(c.h, C.c_int(0), None, None, C.byref(eng), None))
            c._ck(c.L.mdp_aeam_force_host(c.h, C.c_int(0), C.c_int(0), None, None, C.byref(eng), capi._dp(vir), None, None))
    try:
        if style == "rebomos":
            c.rebomos_set_params(ob.product_rebomos_params(R["P"]))
        else:
            c.aeam_set_tables(R["tabs"]); c.aeam_device_lists(True)
        c.set_box_host(s.box)
        c.hnve_setup(spec["dt"], S.FTM2V, s.mass)
        c.langevin_setup(spec["t0"], spec["t1"], spec["damp"], LGV_SEED, n, ratio=LGV_RATIOS[spec["ratio"]], zero=spec["zero"],
                         tally=spec["tally"], boltz=S.BOLTZ, mvv2e=S.MVV2E)
        c.langevin_run(spec["first"], spec["first"] + spec["nsteps"])
        upload(S.wrap(s.box, s.x), v0)
        assert c.host_ghosts_derived()
        compute()
        reads, dev, late_any, rebuilds = dict(spec["reads"]), {}, 0, 0
        for step in range(1, spec["nsteps"] + 1):
            moved, late = c.hnve_initial()
            late_any += int(late)
            if moved or step % rebuild_every == 0:   # the host reneighbours
                got = c.hnve_download(n, want=("x", "v"))
                upload(S.wrap(s.box, got["x"]), got["v"]); rebuilds += 1
            compute()
            c.hnve_final()
            if step in reads:
                got = c.hnve_download(n, want=("x", "v"))
                dev[step] = (got["x"], got["v"], c.langevin_tally())
    finally:
        c.close()
    return dev, late_any, rebuilds


def run_langevin(spec):
    import langevinref
    import mdref
    import refloops
    R = _res()
    s, v0, safe = _lgv_system(spec)
    style, path, skin, nsteps = spec["style"], spec["path"], spec["skin"], spec["nsteps"]
    forced = min(spec["renb"], safe)
    ref_every = min(LGV_REBUILD[style], forced if path in ("resident-plain", "bricks") else safe)
    make = ((lambda sy: mdref.RebomosCPU(R["orc"], R["P"], sy, skin=skin)) if style == "rebomos" else
            (lambda sy: mdref.AeamCPU(R["orc"], R["T"], sy, skin=skin)))
    lgv = langevinref.Langevin(spec["t0"], spec["t1"], spec["damp"], LGV_SEED, s.mass, spec["dt"], S.FTM2V, boltz=S.BOLTZ, mvv2e=S.MVV2E,
                               ratio=LGV_RATIOS[spec["ratio"]], zero=spec["zero"], tally=spec["tally"])
    host = refloops.host_lgv(make, s, v0, nsteps, dict(spec["reads"]), ref_every, lgv, dt=spec["dt"], first=spec["first"], skin=skin)
    err, lim = dict(builds="-", migrated="-"), dict(dx=1e-9, dv=2e-8, de=1e-8)
    if path == "hostlinked":
        dev, late, rebuilds = _lgv_hostlinked(spec, s, v0, ref_every)
        err.update(dangerous=late, builds=rebuilds); lim.update(dangerous=1)
    else:
        dev, left, once, builds, late = _lgv_device(spec, s, v0, spec["ranks"], None if path == "resident" else forced)
        err.update(builds=builds, late=late); lim.update(late=1)
        if path == "bricks":   # and against the one-rank device run of the same case; atoms changed owner, none lost or doubled
            one = _lgv_device(spec, s, v0, 1, forced)[0]
            err.update(dx1=_lgv_worst(s, one, dev, 0), dv1=_lgv_worst(s, one, dev, 1), migrated=left, not_migrated=0 if left > 0 else 1,
                       not_owned_once=0 if once else 1)
            lim.update(dx1=1e-8, dv1=1e-7, not_migrated=1, not_owned_once=1)
    ref = {k: (w[0], w[2], w[1]) for k, w in host.items()}
    err.update(dx=_lgv_worst(s, ref, dev, 0), dv=_lgv_worst(s, ref, dev, 1), de=float(np.abs(np.array([dev[k][2] - ref[k][2] for k in ref])).max()),
               tally_energy=ref[nsteps][2])
    return err, lim


def _lgv_worst(s, a, b, k):
    """the worst difference over the reads of {step: (x, v, ...)}: k = 0 positions (same atom, possibly another image), 1 velocities"""
    import refloops
    worst = 0.0
    for step in a:
        d = b[step][k] - a[step][k]
        if k == 0:
            d = d - np.round(s.box.x2lamda(d + s.box.lo)) @ s.box.h.T
        worst = refloops.worse(worst, float(np.abs(d).max()))     # (a NaN stays, and fails the limit)
    return worst


def line_langevin(spec, err):
    more = "".join(f" {q} {_fmt(err[q])}" for q in ("dx1", "dv1", "dangerous", "late") if q in err)
    return (f"{spec['id']} steps {spec['nsteps']} damp {spec['damp']} ratio {spec['ratio']} zero {int(spec['zero'])} tally {int(spec['tally'])} "
            f"tilt {spec['tilt'] is not None} reads {[(a, int(b)) for a, b in spec['reads']]} drift {spec['drift']} seed {spec['seed']} "
            f"dx {err['dx']:.1e} dv {err['dv']:.1e} dE {err['de']:.1e} (E {err['tally_energy']:.3g}){more} builds {err['builds']} "
            f"migrated {err['migrated']}")


# --------------------------------------------------------------------------------------------------------------- heat
# The constant-flux heat sources (csrc/heat.hip behind every final half) on the three one-rank paths of the integrate
# kernel -- "resident", "resident-plain", "hostlinked" (shuffled host order, host reneighbourings that re-upload atoms,
# velocities and mask); several ranks are refused -- against tests/heatref.host_heat around the ORACLE: 1 - 4 sources on
# group bits drawn from {4, 8, 16, 32, 64} in a shuffled order (slot k does not have the k-th lowest bit), a nevery per
# source from {1, 2, 3, 5, 7} (so the `due` word of a step is empty, partial or full), first steps 0, 1, 7, 1000 and
# 2^32 + 7 (the phase of step % nevery), 40 / 60 / 100 steps of 0.5 / 1 / 2 fs, the integrate group `all` (a mask, but no
# integrate bit) or groupref's, and per source a group shape: every third atom, by tag, of a half of the free atoms, a contiguous
# slab (whole waves of one source), 2 or 3 atoms that are no neighbours, or -- the last source -- the rest of the
# integrate group, so that the sources cover it.  eflux_k = c KEcm_k(0) / dt with c from {0, +-5e-4, +-1e-3, +-3e-3}; one
# source's atoms start with a drift, so that vsub != 0.  Optionally the host starts a second run (mdp_heat_run) at a step
# that is due for some source: that step belongs to the first run; with its final half left pending across the call it
# completes there without the sources, as INTEGRATION.md says.
# At every read: x (minimum image) and v by tag; scale, vcm, ke and the application count of every source's state words
# against the reference's LAST application of that source (a source that was not due at the read step still reports it;
# the count is exact); the atoms outside the integrate group bit for bit; no late check.
# Limits (the reference's, not the device's; both experiments run on the CPU in tests/test_net_draws.py over the suite's
# cases): tests/test_gpu_heat_mdp.py holds the sources to 1e-9 A, 2e-8 A/ps and 1e-12 of the scale.
# With an error of +-1e-9 eV/A on every force component (experiment (ii)) the reference itself moves by 4.6e-10 A,
# 1.3e-8 A/ps and 4.3e-11 of the scale -- more than a quarter of each of those bounds: a tiny group's scale
# sqrt(1 + heat / den) follows its few atoms' velocities --, so for this net each becomes four times the experiment's
# worst: 1.9e-9 A, 5.2e-8 A/ps, 1.8e-10.  The state words vcm and ke had no bound yet: 100 times what the order of a
# source's sum does to them in the reference (experiment (i): 2.14e-14 A/ps, 1.40e-14 relative).
# These five numbers belong to SUITE["heat"]'s seed and case count: they ARE the two experiments' worst over those cases
# (times 4, times 100), and tests/test_net_draws.py compares them with the same experiments, so its margins are thin by
# construction (2.14e-14 < 0.01 * 2.2e-12; 4.56e-10 < 0.25 * 1.9e-9).  Whoever changes the seed, the case count, the draw
# or the rounding of the oracle measures both experiments again (that test prints their worst per quantity) and sets
# the limits and DESIGN.md section 5 from what it prints -- never from what the device gives.
HEAT_PATHS = ("resident", "resident-plain", "hostlinked")
HEAT_FIRST = (0, 1, 7, 1000, 2 ** 32 + 7)
HEAT_BITS = (4, 8, 16, 32, 64)
HEAT_NEVERY = (1, 2, 3, 5, 7)
HEAT_C = (0.0, 5e-4, -5e-4, 1e-3, -1e-3, 3e-3, -3e-3)
HEAT_DRIFT = (0.5, -0.3, 0.2)
HEAT_VCM_LIMIT = 2.2e-12   # A/ps, absolute
HEAT_KE_LIMIT = 1.4e-12    # relative
HEAT_LIMITS = dict(dx=1.9e-9, dv=5.2e-8, dscale=1.8e-10, dvcm=HEAT_VCM_LIMIT, dke=HEAT_KE_LIMIT)


def draw_heat(rng):
    style = rng.choice(["rebomos", "aeam"])
    if style == "rebomos":
        size = rng.choice([(1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 1)])
        spec = dict(size=size, n=_rebo_n(size), frac=None, tilt=None, skin=2.0)
    else:
        size, frac = rng.choice([4, 5, 6, 7]), rng.choice([0.0, 0.03])
        spec = dict(size=size, n=4 * size ** 3, frac=frac, tilt=None, skin=1.0)
        if rng.random() < 0.5:   # a sheared (triclinic) box
            spec["tilt"] = [rng.uniform(-0.06, 0.06) * 4.045 * size for _ in range(3)]
    temp = rng.choice([300.0, 900.0])
    path = rng.choice(HEAT_PATHS)
    nsrc = rng.choice([1, 2, 3, 4])
    bits = list(HEAT_BITS)
    rng.shuffle(bits)
    bits = bits[:nsrc]
    nevery = [rng.choice(HEAT_NEVERY) for _ in range(nsrc)]
    first = rng.choice(HEAT_FIRST)
    nsteps, dt = rng.choice([40, 60, 100]), rng.choice([0.0005, 0.001, 0.002])
    group = rng.choice(["all", "slab"])
    shapes = []
    for k in range(nsrc):
        kind = rng.choice(["modulus", "slab", "tiny", "rest"] if k == nsrc - 1 else ["modulus", "slab", "tiny"])
        axis, width, count, pick = rng.randrange(3), rng.choice([0.15, 0.25]), rng.choice([2, 3]), rng.randrange(10**6)
        shapes.append(dict(kind=kind, axis=axis, width=width, count=count, pick=pick))
    c = [rng.choice(HEAT_C) for _ in range(nsrc)]
    drifting = rng.randrange(nsrc)
    # thermo reads at random steps, the last step among them; True: the read finds the step's final half deferred and
    # completes it (heat pass included), False: the final half ran on its own before the read
    reads = [(st, rng.random() < 0.5) for st in sorted(rng.sample(range(1, nsteps), rng.randint(1, 4))) + [nsteps]]
    cut = None
    if rng.random() < 0.4:   # a second run from a step that is due for source j
        j = rng.randrange(nsrc)
        k = rng.choice([k for k in range(2, nsteps - 1) if (first + k) % nevery[j] == 0])
        pending = rng.random() < 0.5     # the host leaves that step's final half pending across mdp_heat_run
        cut = (k, not pending or path == "hostlinked" or k in dict(reads))
    renb = rng.choice([3, 5, 8])
    spec.update(style=style, temp=temp, path=path, nsrc=nsrc, bits=bits, nevery=nevery, first=first, nsteps=nsteps, dt=dt, group=group,
                shapes=shapes, c=c, drifting=drifting, reads=reads, cut=cut, renb=renb, seed=rng.randrange(1, 10**6), env={},
                id=f"{style}-{path}-n{spec['n']}-{group}-src{nsrc}-every{'.'.join(map(str, nevery))}-first{first}-dt{dt}"
                   + (f"-cut{cut[0]}{'' if cut[1] else 'p'}" if cut else ""))
    return spec


def heat_due(spec, step):
    """the `due` word of run step `step`: bit k set if source k is applied behind it"""
    if spec["cut"] is not None and step == spec["cut"][0] and not spec["cut"][1]:
        return 0
    return sum(1 << k for k, ne in enumerate(spec["nevery"]) if (spec["first"] + step) % ne == 0)


def _heat_system(spec):
    """no GPU, no oracle: (system, start velocities with the drift, mask by tag, integrate group, [group of source k],
    [eflux of source k], the steps between forced list builds by the _lgv_system rule)"""
    import groupref
    import heatref
    af = _res()["af"]
    if spec["style"] == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), spec["size"])
    else:
        s = S.fcc_cell(4.045, spec["size"], frac_type2=spec["frac"], seed=spec["seed"]); s.mass[1:3] = af.mass[:2]
        if spec["tilt"] is not None:
            # the sites a quarter of the lattice constant off the box faces: a site ON a face of a sheared box has a lamda
            # coordinate that rounds to just outside at some builds, and the remap rewrites every atom that left the box,
            # held ones included, by a box vector -- the held atoms could not be compared bit for bit then
            nb = S.Box(s.box.lo.copy(), s.box.prd.copy(), np.array(spec["tilt"]))
            s = S.System(nb, nb.lamda2x(s.box.x2lamda(s.x) + 0.25 / spec["size"]), s.type, s.tag, s.mass)
    assert s.n == spec["n"]
    lam = s.box.x2lamda(S.wrap(s.box, s.x))
    g = np.ones(s.n, dtype=bool) if spec["group"] == "all" else groupref.masks(s)[1]
    free, groups = g.copy(), []
    for k, sh in enumerate(spec["shapes"]):
        a = lam[:, sh["axis"]]
        if sh["kind"] == "modulus":    # every third, in the order of the tags, of the upper half, along the axis, of the atoms still
            up = free & (a >= np.median(a[free]))     # free: lanes of a wave alternate between this source and others
            l = up & (np.cumsum(up) % 3 == 0)
        elif sh["kind"] == "slab":     # contiguous: of the integrate group's atoms in their order along the axis, those from
            rank = np.empty(s.n)       # k / 4 on, `width` of them -- whole planes of the crystal, a plane cut at the ends
            rank[np.argsort(np.where(g, a, np.inf), kind="stable")] = np.arange(s.n) / g.sum()
            l = free & (rank >= 0.25 * k) & (rank < 0.25 * k + sh["width"])
        elif sh["kind"] == "rest":
            l = free.copy()
        else:                          # 2 or 3 atoms, no two of them within 6 A of each other
            r = np.random.default_rng(sh["pick"])
            l = np.zeros(s.n, dtype=bool)
            for i in r.permutation(np.flatnonzero(free)):
                d = s.x[l] - s.x[i]
                d = d - np.round(s.box.x2lamda(d + s.box.lo)) @ s.box.h.T
                if not l.any() or float(np.sqrt((d ** 2).sum(axis=1)).min()) > 6.0:
                    l[i] = True
                if l.sum() == sh["count"]:
                    break
        assert l.sum() >= 2, (spec["id"], k, sh["kind"], int(l.sum()))
        groups.append(l)
        free &= ~l
    by_tag = np.zeros(int(s.tag.max()) + 1, dtype=np.int32)
    m = groupref.ALL_BIT | np.where(g, groupref.INTEGRATE_BIT, 0)
    for bit, l in zip(spec["bits"], groups):
        m = m | np.where(l, bit, 0)
    by_tag[s.tag] = m
    v0 = S.gaussian_velocities(s, spec["temp"], seed=spec["seed"] + 1)
    v0[groups[spec["drifting"]]] += np.array(HEAT_DRIFT)
    mass = s.mass[s.type]
    flux = [c * heatref.kecm(v0, mass, l, S.FTM2V, S.MVV2E) * S.MVV2E / spec["dt"] for c, l in zip(spec["c"], groups)]
    vcap = float(np.sqrt((v0 ** 2).sum(axis=1)).max()) + 5.0 * np.sqrt(S.BOLTZ * 1.5 * spec["temp"] / (float(s.mass[1:3].min()) * S.MVV2E))
    safe = max(1, int(0.3 * spec["skin"] / (vcap * spec["dt"])))
    return s, v0, by_tag, g, groups, flux, safe


def _heat_intervals(spec, safe):
    """(the interval of the device's forced builds on "resident-plain"; the interval of the reference's builds and of the
    host's reneighbourings on "hostlinked": refloops.host_lgv's rule, a fixed interval shortened to what is safe)"""
    return min(spec["renb"], safe), min(LGV_REBUILD[spec["style"]], safe)


def heat_reference(spec, permuted=False, dforce=0.0):
    """no GPU: heatref.host_heat of the case around the oracle; ({read step: (x, scales, v, states)}, lowest escale).
    permuted: every source's atoms summed in a random order (experiment (i)); dforce: experiment (ii)"""
    import heatref
    import mdref
    R = _res()
    s, v0, by_tag, g, groups, flux, safe = _heat_system(spec)
    skin = spec["skin"]
    make = ((lambda sy: mdref.RebomosCPU(R["orc"], R["P"], sy, skin=skin)) if spec["style"] == "rebomos" else
            (lambda sy: mdref.AeamCPU(R["orc"], R["T"], sy, skin=skin)))
    sources = [dict(group=l, eflux=fl, nevery=ne) for l, fl, ne in zip(groups, flux, spec["nevery"])]
    orders = None
    if permuted:
        r = np.random.default_rng(spec["seed"] + 2)
        orders = [r.permutation(int(l.sum())) for l in groups]
    return heatref.host_heat(make, s, v0, spec["nsteps"], dict(spec["reads"]), _heat_intervals(spec, safe)[1], g, sources, dt=spec["dt"],
                             orders=orders, first=spec["first"], cut=spec["cut"], skin=skin, dforce=dforce, states=True)


def heat_worst(spec, s, g, ref, dev, x_in=None, v_in=None):
    """the worst deviations of {step: (x, scales, v, states)} `dev` from `ref` over the reads; with x_in / v_in also
    whether an atom outside the integrate group changed (held) and whether an application count differs (count)"""
    import refloops
    w = dict(dx=0.0, dv=0.0, dscale=0.0, dvcm=0.0, dke=0.0)
    held = count = 0
    for step in ref:
        xh, _, vh, sth = ref[step]
        xd, _, vd, std = dev[step]
        d = xd - xh
        d = d - np.round(s.box.x2lamda(d + s.box.lo)) @ s.box.h.T
        w["dx"] = refloops.worse(w["dx"], float(np.abs(d).max()))
        w["dv"] = refloops.worse(w["dv"], float(np.abs(vd - vh).max()))
        for a, b in zip(std, sth):
            w["dscale"] = refloops.worse(w["dscale"], abs(a["scale"] - b["scale"]) / abs(b["scale"]))
            w["dvcm"] = refloops.worse(w["dvcm"], float(np.abs(a["vcm"] - b["vcm"]).max()))
            w["dke"] = refloops.worse(w["dke"], abs(a["kecm"] - b["kecm"]) / abs(b["kecm"]) if b["kecm"] else abs(a["kecm"]))
            count += int(a["applied"] != b["applied"])
        if x_in is not None:
            held += int(not (np.array_equal(xd[~g], x_in[~g]) and np.array_equal(vd[~g], v_in[~g])))
    if x_in is not None:
        w.update(held=held, count=count)
    return w


def _heat_states(ctx, nsrc):
    return [dict(scale=q["scale"], vcm=q["vcm"], kecm=q["kecm"], applied=q["applied"]) for q in (ctx.heat_state(k) for k in range(nsrc))]


def _heat_resident(spec, s, v0, by_tag, g, dsrc, rebuild_every):
    """one resident brick.  rebuild_every None: the device's own check; a number: the integrate calls without the check,
    reneighbourings forced every so many steps.  The reads go through the library (mdp_heat_state completes a deferred
    final half, heat pass included), not through DeviceDomain.flush"""
    import groupref
    from lammps_plugins_amd.host import resident
    reads, cut = dict(spec["reads"]), spec["cut"]
    ctx, st, cutghost, map_ = _lgv_context(spec["style"])
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, spec["skin"], map_, v0=v0, dt=spec["dt"])
        d.set_group(by_tag, 0 if spec["group"] == "all" else groupref.INTEGRATE_BIT)
        d.heat(dsrc, first=spec["first"])
        d.compute(1, 0)
        out = {}
        for step in range(1, spec["nsteps"] + 1):
            rb = "auto" if rebuild_every is None else step % rebuild_every == 0
            defer = reads.get(step, True)
            if cut is not None and step == cut[0] and step not in reads:
                defer = not cut[1]
            d.step(0, 0, rebuild=rb, defer_final=defer)
            if step in reads:
                sts = _heat_states(ctx, spec["nsrc"])
                got = ctx.md_download(d.nlocal, want=("x", "v"))
                x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
                x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
                out[step] = (x, [q["scale"] for q in sts], v, sts)
            if cut is not None and step == cut[0]:
                d.heat_run(spec["first"] + step)         # (completes a pending final half, without the sources)
        return out, d.builds, d.dangerous
    finally:
        ctx.close()


def _heat_hostlinked(spec, s, v0, by_tag, g, dsrc, rebuild_every):
    """mdp_hnve_* with mdp_hnve_set_mask from a shuffled host order; a host reneighbouring (every rebuild_every steps and
    whenever mdp_hnve_initial reports `moved`) downloads, wraps the integrated atoms and uploads atoms, velocities and
    mask again"""
    import ctypes as C
    import groupref
    import oracle_bindings as ob
    from lammps_plugins_amd.host import capi
    R = _res()
    style, n, skin = spec["style"], s.n, spec["skin"]
    cut = (R["P"].cut3rebo if style == "rebomos" else float(R["af"].cut_table(R["tabs"]).max())) + skin
    perm = np.random.default_rng(spec["seed"] + 3).permutation(n)
    type_p, tag_p, gp = s.type[perm].copy(), s.tag[perm].copy(), g[perm]
    mask_p = by_tag[tag_p]
    c = capi.Context(0)

    def upload(x, v):
        xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), type_p, tag_p, s.mass), cut)
        c.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=[0, 0, 1] if style == "rebomos" else None)
        c.set_skin(skin)
        c.hnve_upload_v(v)

    def compute():   # f == NULL: the forces' only reader is the device's integrator
        if style == "rebomos":
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
        else:
            eng, vir = C.c_double(0.0), np.zeros(6)
            c._ck(c.L.mdp_aeam_density_host(c.h, C.c_int(0), None, None, C.byref(eng), None))
            c._ck(c.L.mdp_aeam_force_host(c.h, C.c_int(0), C.c_int(0), None, None, C.byref(eng), capi._dp(vir), None, None))
    try:
        if style == "rebomos":
            c.rebomos_set_params(ob.product_rebomos_params(R["P"]))
        else:
            c.aeam_set_tables(R["tabs"]); c.aeam_device_lists(True)
        c.set_box_host(s.box)
        c.hnve_setup(spec["dt"], S.FTM2V, s.mass)
        c.integrate_group(0 if spec["group"] == "all" else groupref.INTEGRATE_BIT)
        upload(S.wrap(s.box, s.x)[perm], v0[perm])
        c.hnve_set_mask(mask_p)
        c.heat_setup(dsrc, mvv2e=S.MVV2E)
        c.heat_run(spec["first"])
        compute()
        reads, out, late_any, rebuilds = dict(spec["reads"]), {}, 0, 0
        for step in range(1, spec["nsteps"] + 1):
            moved, late = c.hnve_initial()
            late_any += int(late)
            if moved or step % rebuild_every == 0:
                got = c.hnve_download(n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]     # (a host that wraps rewrites only atoms that left the box: the held ones did not)
                upload(xw, got["v"])
                c.hnve_set_mask(mask_p)
                rebuilds += 1
            compute()
            c.hnve_final()
            if step in reads:
                sts = _heat_states(c, spec["nsrc"])
                got = c.hnve_download(n, want=("x", "v"))
                x, v = np.zeros((n, 3)), np.zeros((n, 3))
                x[tag_p - 1], v[tag_p - 1] = got["x"], got["v"]
                out[step] = (x, [q["scale"] for q in sts], v, sts)
            if spec["cut"] is not None and step == spec["cut"][0]:
                c.heat_run(spec["first"] + step)
    finally:
        c.close()
    return out, rebuilds, late_any


def run_heat(spec):
    s, v0, by_tag, g, groups, flux, safe = _heat_system(spec)
    forced, ref_every = _heat_intervals(spec, safe)
    ref, lowest = heat_reference(spec)
    dsrc = [dict(eflux=fl, nevery=ne, bit=b) for fl, ne, b in zip(flux, spec["nevery"], spec["bits"])]
    if spec["path"] == "hostlinked":
        dev, builds, late = _heat_hostlinked(spec, s, v0, by_tag, g, dsrc, ref_every)
    else:
        dev, builds, late = _heat_resident(spec, s, v0, by_tag, g, dsrc, None if spec["path"] == "resident" else forced)
    # The atoms outside the integrate group keep, bit for bit, the positions (wrapped into the box, as every path uploads
    # them) and the velocities they were given
    err = heat_worst(spec, s, g, ref, dev, S.wrap(s.box, s.x), v0)
    err.update(late=late, builds=builds, lowest=lowest, sizes=[int(l.sum()) for l in groups],
               applied=[q["applied"] for q in dev[spec["nsteps"]][3]])
    return err, dict(HEAT_LIMITS, held=1, count=1, late=1)


def line_heat(spec, err):
    return (f"{spec['id']} steps {spec['nsteps']} T {spec['temp']:.0f} bits {spec['bits']} shapes {[q['kind'] for q in spec['shapes']]} sizes {err['sizes']} "
            f"c {spec['c']} drifting {spec['drifting']} tilt {spec['tilt'] is not None} reads {[(a, int(b)) for a, b in spec['reads']]} "
            f"seed {spec['seed']} dx {err['dx']:.1e} dv {err['dv']:.1e} scale {err['dscale']:.1e} vcm {err['dvcm']:.1e} ke {err['dke']:.1e} "
            f"applied {err['applied']} count {err['count']} held {err['held']} late {err['late']} lowest escale {err['lowest']:.4f} "
            f"builds {err['builds']}")


# ------------------------------------------------------------------------------------------------------------ measure
# compute rdf/mdp and compute adf/mdp (csrc/rdf.hip, csrc/adf.hip behind csrc/measure_bin.hip), both set up on one context
# per rank, against the brute-force references tests/rdfref.py and tests/adfref.py on positions merged by tag from the same
# run: MoS2 replicas (1,1,1) - (2,2,2) or the alloy at 5 - 8 cells (sheared in some cases, relabelled to 3 - 12 types in
# some), jittered and at 300 - 2 500 K, some with a drift; 1, 2, 3, 4 or 8 bricks of the thread transport, a free dimension
# in some one-brick alloy cases; no group, a slab, a modulus class of the tags, 2 - 3 atoms or every atom of one type left
# out; 1 - 32 columns and triples with random type ranges, 1 - 8192 / columns bins, cutoffs from just above the first
# shell (where the cap of bin_grid widens the cells) to cutghost - skin, shells with random radii (no centre with more
# than 100 neighbours at the start: the cap is 128), every ordinate; MDP_MEASURE_GRID unset or 1, 3, 64 (a workgroup
# then walks several chunks and, at 1, flushes inside its loop).  Reads at step 0, in between and at the end, each taken
# twice.  The references bracket in integers, so there is no tolerance: every error is a count that must be 0, except the
# reference's own edge events (pairs and angles within 1e-9 of a bin edge, neighbours at a shell radius), which the fixed
# tests cap at 2.  A case that is not about a tiny group holds at least 1e4 rdf entries and 1e4 angles at every read.
MSR_NPAIR = (1, 2, 5, 17, 32)
MSR_NTRIPLE = (1, 3, 8, 32)
MSR_NBIN = (1, 2, 37, 50, 200, 1000, None)      # None: 8192 // columns, the whole LDS histogram
MSR_COUNTERS = 8192
MSR_GROUPS = ("none", "slab", "modulus", "tiny", "one type out")
MSR_ORDINATES = ("degree", "radian", "cosine")
MSR_GRID = ("1", "3", "64")
MSR_FIRST = {"rebomos": 2.41, "aeam": 2.86}      # first shell: the Mo-S bond, fcc nearest neighbours
MSR_LIMIT = {"rebomos": 11.4, "aeam": 6.5}       # cutghost - skin of the bundled potentials (run_measure asserts it)
MSR_SKIN = {"rebomos": 2.0, "aeam": 1.0}
MSR_NEIGH = 100                                  # neighbours of a centre inside the largest outer radius, at the start
MSR_FLOOR, MSR_FLOOR_START = 10 ** 4, 3 * 10 ** 4   # entries and angles of a read; what the draw asks of the start positions
MSR_EDGE_LIMIT = 3
_MSR_DRAWN = {}


def measure_bin_grid(lens, cutoff, nall):
    """bin_grid of csrc/measure_bin.hip restated: (cells per dimension, how often the cell width grew by 1.26 from
    cutoff / 2) over a bounding box with edge lengths lens for nall atoms"""
    binsize, cap, grown = 0.5 * cutoff, 4 * nall + 4096, 0
    while True:
        n = [min(1024, max(1, int(np.floor(l / binsize)))) for l in lens]
        if n[0] * n[1] * n[2] <= cap:
            return n, grown
        binsize *= 1.26
        grown += 1


def measure_domain_lens(box, cutghost):
    """the edge lengths of the bounding box DeviceDomain sets: the box's corners, cutghost + 2 A further each way.  (On one
    brick the hull the library sets at a reneighbouring holds this box, so a cell count over it is a lower bound.)"""
    corners = box.lamda2x(np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=float))
    return [float(corners[:, d].max() - corners[:, d].min() + 2.0 * (cutghost + 2.0)) for d in range(3)]


def measure_nall_bound(box, n, cutghost, nonperiodic=(0, 0, 0)):
    """an upper bound of nlocal + nghost on one brick from the density: the atoms of the box and its images inside the
    ghost shell, lamda from -cutghost / width to 1 + cutghost / width in every periodic dimension, and 5 % more"""
    hinv = np.linalg.inv(box.h)
    f = 1.0
    for d in range(3):
        if not nonperiodic[d]:
            f *= 1.0 + 2.0 * cutghost * float(np.linalg.norm(hinv[d]))
    return int(np.ceil(1.05 * n * f))


def measure_grid_grows(spec, cutoff=None):
    """no GPU: the first trial grid of a read of a one-brick case (cutoff None: the rdf read of a `measure` case), cells
    cutoff / 2 wide, exceeds bin_grid's cap"""
    cutoff = spec["cutoff"] if cutoff is None else cutoff
    if spec["ranks"] != 1 or cutoff is None:
        return False
    box = _cell_start(spec).box
    cutghost = MSR_LIMIT[spec["style"]] + MSR_SKIN[spec["style"]]
    nall = measure_nall_bound(box, spec["n"], cutghost, spec["nonperiodic"])
    return measure_bin_grid(measure_domain_lens(box, cutghost), cutoff, nall)[1] > 0


def _msr_range(rng, nt):
    lo = rng.randint(1, nt)
    return lo, rng.randint(lo, nt)


def draw_measure(rng):
    key = rng.getstate()
    if key in _MSR_DRAWN:     # (the geometry below costs seconds; the draw is a function of the generator's state)
        import copy
        spec, after = _MSR_DRAWN[key]
        rng.setstate(after)
        return copy.deepcopy(spec)
    import copy
    spec = _msr_random(rng)
    _msr_fit(spec)
    _MSR_DRAWN[key] = (copy.deepcopy(spec), rng.getstate())
    return spec


def _msr_random(rng):
    """the draws of a case; _msr_fit then bounds the radii and meets the floors on the start positions without drawing"""
    style = rng.choice(["rebomos", "aeam"])
    sd = rng.randrange(1, 10**6)
    spec = dict(style=style, seed=sd, tilt=None, relabel=None, frac=None, nonperiodic=(0, 0, 0))
    if style == "rebomos":
        size = (rng.choice([1, 2]), rng.choice([1, 2]), rng.choice([1, 2]))
        spec.update(size=size, n=_rebo_n(size), ntypes=2)
    else:
        size = rng.choice([5, 6, 7, 8])
        spec.update(size=size, n=4 * size ** 3, ntypes=2, frac=rng.choice([0.05, 0.2, 0.5]))
        if rng.random() < 0.4:   # a sheared (triclinic) box, as draw_force shears it
            spec["tilt"] = [rng.uniform(-0.12, 0.12) * 4.045 * size for _ in range(3)]
        if rng.random() < 0.5:   # relabelled to 3 - 12 types, as run_aeam_types relabels it
            spec["relabel"] = rng.choice([(2, 1), (3, 2), (4, 2), (5, 3), (7, 5), (1, 3), (6, 2)])
            spec["ntypes"] = sum(spec["relabel"])
    nt = spec["ntypes"]
    spec["amp"] = rng.choice([0.02, 0.05, 0.08])
    spec["temp"] = rng.choice([300, 1200, 2500])
    spec["drift"] = [rng.choice([-60, -30, 0, 25, 40, 70]) for _ in range(3)] if rng.random() < 0.4 else [0, 0, 0]
    spec["nsteps"] = rng.randint(5, 40)
    spec["ranks"] = 1 if rng.random() < 0.5 else rng.choice([2, 3, 4, 8])
    auto, renb = rng.random() < 0.5, rng.choice([3, 5, 8])
    spec["rebuild"] = "auto" if auto and spec["ranks"] == 1 else renb     # (the device's own check serves one brick only)
    free = rng.random() < 0.4, rng.randrange(3)
    if style == "aeam" and spec["ranks"] == 1 and spec["tilt"] is None and free[0]:
        spec["nonperiodic"] = tuple(int(d == free[1]) for d in range(3))
        spec["drift"] = [0, 0, 0]
    spec["between"] = rng.randint(1, spec["nsteps"] - 1)
    kind = rng.choice(MSR_GROUPS)
    spec["group"] = dict(kind=kind, axis=rng.randrange(3), lo=rng.uniform(0.0, 0.5), width=rng.uniform(0.3, 0.5), m=rng.choice([2, 3, 5]),
                         r=rng.randrange(2), count=rng.choice([2, 3]), pick=rng.randrange(10**6), type=rng.randint(1, nt))
    first, limit = MSR_FIRST[style], MSR_LIMIT[style]
    # ---- rdf
    npair = rng.choice(MSR_NPAIR)
    spec["pairs"] = [_msr_range(rng, nt) + _msr_range(rng, nt) for _ in range(npair)]
    nbin = rng.choice(MSR_NBIN)
    spec["nbin_rdf"] = MSR_COUNTERS // npair if nbin is None else min(nbin, MSR_COUNTERS // npair)     # (1000 x 17 is refused)
    u, small, a, b = rng.random(), rng.random() < 0.4, rng.uniform(1.02, 1.15), rng.uniform(1.02 * first, 0.999 * limit)
    spec["cutoff"] = None if u < 1.0 / 3.0 else (a * first if small else b)       # None: the limit cutghost - skin
    spec["small"] = spec["cutoff"] is not None and small
    # ---- adf; the outer radii are fractions here, of first .. the radius that holds MSR_NEIGH neighbours (_msr_fit)
    ntriple = rng.choice(MSR_NTRIPLE)
    spec["triples"] = []
    for _ in range(ntriple):
        row = _msr_range(rng, nt) + _msr_range(rng, nt) + _msr_range(rng, nt)
        for _shell in range(2):
            near, out = rng.random() < 0.7, rng.random()
            inner = 0.0 if rng.random() < 0.6 else rng.uniform(0.0, 0.8)
            row += (inner, (0.25 * out) if near else out)        # (inner as a fraction of the outer radius)
        spec["triples"].append(row)
    nbin = rng.choice(MSR_NBIN)
    spec["nbin_adf"] = MSR_COUNTERS // ntriple if nbin is None else min(nbin, MSR_COUNTERS // ntriple)
    spec["ordinate"] = rng.choice(MSR_ORDINATES)
    spec["env"] = {"MDP_MEASURE_GRID": rng.choice(MSR_GRID)} if rng.random() < 0.5 else {}
    return spec


def _cell_start(spec):
    """no GPU, no oracle: the start system of a case, jittered (placeholder masses; run_measure sets the potential's)"""
    sd = spec["seed"]
    if spec.get("cell"):      # a constructed cell of tests/cnaref.py (the structure net): one type of the alloy's, its own jitter
        import cnaref
        x, h = {"stack": lambda: cnaref.stack_cell(spec["amp"], sd)[:2], "bcc": lambda: cnaref.bcc_cell(sigma=spec["amp"], seed=sd),
                "icosahedron": lambda: cnaref.icosahedron_cell(spec["amp"], sd)}[spec["cell"]]()
        box = S.Box(np.zeros(3), np.asarray(h).diagonal().copy(), np.zeros(3))
        assert len(x) == spec["n"]
        return S.System(box, S.wrap(box, x), np.ones(len(x), dtype=np.int32), np.arange(1, len(x) + 1, dtype=np.int32), np.array([0.0, 27.0, 28.0]))
    if spec["style"] == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), spec["size"])
    else:
        s = S.fcc_cell(4.045, spec["size"], frac_type2=spec["frac"], seed=sd)
        if spec["tilt"] is not None:
            nb = S.Box(s.box.lo.copy(), s.box.prd.copy(), np.array(spec["tilt"]))
            s = S.System(nb, nb.lamda2x(s.box.x2lamda(s.x)), s.type, s.tag, s.mass)
        if spec["relabel"] is not None:
            nmet, nang = spec["relabel"]
            r = np.random.default_rng(sd)
            ty = np.where(s.type == 1, r.integers(1, nmet + 1, s.n), r.integers(nmet + 1, nmet + nang + 1, s.n)).astype(np.int32)
            s = S.System(s.box, s.x, ty, s.tag, np.array([0.0] + [27.0] * nmet + [28.0] * nang))
    assert s.n == spec["n"] and np.array_equal(s.tag, np.arange(1, s.n + 1))
    return S.jitter(s, spec["amp"], seed=sd + 1)


def _cell_periodic(spec):
    return tuple(0 if f else 1 for f in spec["nonperiodic"])


def _msr_pairs(s, spec, rmax):
    import rdfref
    out = list(rdfref._pairs_in_range(np.ascontiguousarray(s.x), s.box.h, _cell_periodic(spec), rmax))
    if not out:
        return np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0)
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def group_member(spec, s, pairs=None):
    """the member table of the case by tag (row t - 1), or None; s: the start system.  A tiny group is an atom and one or
    two of its nearest neighbours, so that it holds a pair"""
    g = spec["group"]
    if g["kind"] == "none":
        return None
    if g["kind"] == "slab":
        a = s.box.x2lamda(s.x)[:, g["axis"]]
        return (a >= g["lo"]) & (a < g["lo"] + g["width"])
    if g["kind"] == "modulus":
        return s.tag % g["m"] == g["r"]
    if g["kind"] == "one type out":
        return s.type != g["type"]
    if "tags" not in g:
        pi, pj, pr = _msr_pairs(s, spec, 1.25 * MSR_FIRST[spec["style"]]) if pairs is None else pairs
        r = np.random.default_rng(g["pick"])
        i = int(r.integers(0, s.n))
        near = pj[(pi == i) & (pr < 1.25 * MSR_FIRST[spec["style"]])]
        near = np.unique(near[near != i])
        g["tags"] = sorted(int(t) for t in [i + 1] + (r.permutation(near)[:g["count"] - 1] + 1).tolist())
    m = np.zeros(s.n, dtype=bool)
    m[np.array(g["tags"]) - 1] = True
    return m


def _msr_in(t, lo, hi):
    return (t >= lo) & (t <= hi)


def measure_start_counts(spec, s, member, pairs):
    """(rdf entries, angles) of the case on its start positions from the pair list (i, j, r): exact counts, summed over columns"""
    pi, pj, pr = pairs
    t = s.type
    mem = np.ones(s.n, dtype=bool) if member is None else member
    both = mem[pi] & mem[pj]
    cutoff = MSR_LIMIT[spec["style"]] if spec["cutoff"] is None else spec["cutoff"]
    entries = sum(int((both & (pr < cutoff) & _msr_in(t[pi], p[0], p[1]) & _msr_in(t[pj], p[2], p[3])).sum()) for p in spec["pairs"])
    angles = 0
    for tr in spec["triples"]:
        c = both & _msr_in(t[pi], tr[0], tr[1])
        jq = c & _msr_in(t[pj], tr[2], tr[3]) & (pr >= tr[6]) & (pr < tr[7])
        kq = c & _msr_in(t[pj], tr[4], tr[5]) & (pr >= tr[8]) & (pr < tr[9])
        nj, nk, njk = (np.bincount(pi[q], minlength=s.n) for q in (jq, kq, jq & kq))
        angles += int((nj * nk - njk).sum())
    return entries, angles


def _cell_rcap(s, pairs, limit):
    """no draws: the radius inside which no centre has more than MSR_NEIGH neighbours at the start, at most the limit: from the
    distance of every centre's neighbour number MSR_NEIGH + 1, if it lies inside the limit"""
    pi, pj, pr = pairs
    order = np.lexsort((pr, pi))
    start = np.searchsorted(pi[order], np.arange(s.n + 1))
    full = np.nonzero(np.diff(start) > MSR_NEIGH)[0]
    rcap = 0.999 * limit
    if len(full):
        rcap = min(rcap, 0.999 * float(pr[order][start[full] + MSR_NEIGH].min()))
    return rcap


def _msr_fit(spec):
    """no draws: turns the triples' fractions into radii -- between the first shell and the radius inside which no centre
    has more than MSR_NEIGH neighbours at the start (at most the limit) --, and, for a case that is not about a tiny group,
    meets MSR_FLOOR_START entries and angles on the start positions: first column 1 / triple 1 over all types, then the
    cutoff at the limit and triple 1 over the widest shell, then no group"""
    style, nt = spec["style"], spec["ntypes"]
    first, limit = MSR_FIRST[style], MSR_LIMIT[style]
    s = _cell_start(spec)
    pairs = _msr_pairs(s, spec, limit)
    rcap = _cell_rcap(s, pairs, limit)
    rows = []
    for tr in spec["triples"]:
        row = list(tr[:6])
        for k in (6, 8):
            rout = 1.05 * first + tr[k + 1] * (rcap - 1.05 * first)
            row += [tr[k] * rout, rout]
        rows.append(tuple(float(v) if k >= 6 else int(v) for k, v in enumerate(row)))
    spec["triples"] = rows
    spec["rcap"] = float(rcap)
    member = group_member(spec, s, pairs)
    exempt = spec["group"]["kind"] in ("tiny", "one type out")
    steps = ("all types", "widest", "no group")
    spec["fitted"] = []
    if exempt:      # column 1 and triple 1 over all types, so that the few members, or the columns without a centre, stand next to counts
        spec["pairs"][0] = (1, nt, 1, nt)
        spec["triples"][0] = (1, nt, 1, nt, 1, nt) + spec["triples"][0][6:]
    while not exempt:
        entries, angles = measure_start_counts(spec, s, member, pairs)
        if (entries >= MSR_FLOOR_START and angles >= MSR_FLOOR_START) or len(spec["fitted"]) == len(steps):
            break
        step = steps[len(spec["fitted"])]
        spec["fitted"].append(step)
        if step == "all types":
            spec["pairs"][0] = (1, nt, 1, nt)
            spec["triples"][0] = (1, nt, 1, nt, 1, nt) + spec["triples"][0][6:]
        elif step == "widest":
            spec["cutoff"], spec["small"] = None, False
            spec["triples"][0] = spec["triples"][0][:6] + (0.0, spec["rcap"], 0.0, spec["rcap"])
        else:
            spec["group"]["kind"], member = "none", None
    g = spec["group"]["kind"].replace(" ", "")
    spec["id"] = (f"{style}-n{spec['n']}-types{nt}-ranks{spec['ranks']}-{g}-rdf{len(spec['pairs'])}x{spec['nbin_rdf']}-"
                  f"adf{len(spec['triples'])}x{spec['nbin_adf']}-{spec['ordinate']}-grid{spec['env'].get('MDP_MEASURE_GRID', 'unset')}")


def _cell_speed_cap(spec, s, v0):
    """the speed no atom is expected to exceed during the run: the fastest atom of the start and five thermal standard
    deviations of the lightest type more (of 300 K for a colder start, whose atoms the jitter's forces set moving)"""
    return float(np.sqrt((v0 ** 2).sum(axis=1)).max()) + 5.0 * np.sqrt(S.BOLTZ * max(spec["temp"], 300) / (float(s.mass[1:].min()) * S.MVV2E))


def _cell_velocities(spec, s):
    """start velocities (with the drift; exactly zero at 0 K) and the steps between forced list builds by the _lgv_system rule"""
    if spec["temp"] == 0:
        v0 = np.zeros((s.n, 3))
    else:
        v0 = S.gaussian_velocities(s, float(spec["temp"]), seed=spec["seed"] + 2) + np.array(spec["drift"], dtype=float)
    return v0, max(1, int(0.3 * MSR_SKIN[spec["style"]] / (_cell_speed_cap(spec, s, v0) * 0.001)))


def _cell_potential(spec, s):
    """the potential of a case: sets the masses of s; (the alloy's tables or None, cutghost).  cutghost - skin is MSR_LIMIT"""
    import aeam_five
    from lammps_plugins_amd.host import capi
    R = _res()
    style, skin = spec["style"], MSR_SKIN[spec["style"]]
    tabs = None
    if style == "rebomos":
        cutghost = 3.0 * R["rp"].rcmax[0][0] + skin
    else:
        af, tabs = R["af"], R["tabs"]
        if spec["relabel"] is not None:
            nmet, nang = spec["relabel"]
            if "tmp" not in R:
                R["tmp"] = tempfile.mkdtemp()
            path = os.path.join(R["tmp"], f"p{nmet}_{nang}.aeam")
            if not os.path.exists(path):
                aeam_five.write_relabelled_file(path, R["pot_aeam"], [0] * nmet + [1] * nang, ["M%d" % i for i in range(nmet)] + ["X%d" % i for i in range(nang)])
            if path not in R:     # (kept for the process: the tables point into the file object, which frees them when it goes)
                af = capi.AeamFile(path)
                R[path] = (af, af.build())
            af, tabs = R[path]
        s.mass[1:] = af.mass[:spec["ntypes"]]
        cutghost = float(af.cut_table(tabs).max()) + skin
    assert abs(cutghost - skin - MSR_LIMIT[style]) < 1e-9, cutghost - skin
    return tabs, cutghost


def _cell_domain(spec, s, tabs, cutghost, v0, make_tr):
    """(context, DeviceDomain) of one rank of a case; the caller closes the context"""
    from lammps_plugins_amd.host import capi, resident
    ctx = capi.Context(0)
    try:
        if spec["style"] == "rebomos":
            ctx.rebomos_set_params(_res()["rp"])
            st, map_ = capi.STYLE_REBOMOS, [0, 0, 1]
        else:
            ctx.aeam_set_tables(tabs)
            st, map_ = capi.STYLE_AEAM, None
        return ctx, resident.DeviceDomain(ctx, st, s, cutghost, MSR_SKIN[spec["style"]], map_, v0=v0,
                                          transport=make_tr(ctx) if spec["ranks"] > 1 else None, nonperiodic=spec["nonperiodic"])
    except BaseException:
        ctx.close()
        raise


def measure_references(spec, x, types, h, member):
    """rdfref.counts and adfref.counts of the case on positions and types by tag"""
    import adfref
    import rdfref
    per = _cell_periodic(spec)
    cutoff = spec.get("cutoff_used") or spec["cutoff"] or MSR_LIMIT[spec["style"]]
    return (rdfref.counts(x, types, h, per, cutoff, spec["nbin_rdf"], spec["pairs"], member),
            adfref.counts(x, types, h, per, spec["nbin_adf"], spec["ordinate"], spec["triples"], member))


def _msr_outside(hist, ref):
    low, high = ref["hist_sure"], ref["hist_sure"] + ref["edge_adjacent"]
    return int(((hist < low) | (hist > high)).sum())


def run_measure(spec):
    from lammps_plugins_amd.host import resident
    style = spec["style"]
    s = _cell_start(spec)
    tabs, cutghost = _cell_potential(spec, s)
    limit = MSR_LIMIT[style]
    cutoff = limit if spec["cutoff"] is None else spec["cutoff"]
    member = group_member(spec, s)
    v0, safe = _cell_velocities(spec, s)
    rebuild = spec["rebuild"] if spec["rebuild"] == "auto" else min(spec["rebuild"], safe)
    reads = sorted({0, spec["between"], spec["nsteps"]})
    pairs = [((p[0], p[1]), (p[2], p[3])) for p in spec["pairs"]]
    triples = [((t[0], t[1]), (t[2], t[3]), (t[4], t[5])) + tuple(t[6:]) for t in spec["triples"]]
    world = spec["ranks"]

    def rank_fn(r, make_tr):
        ctx, d = _cell_domain(spec, s, tabs, cutghost, v0, make_tr)
        try:
            d.rdf(spec["nbin_rdf"], cutoff, pairs, member_by_tag=member)
            d.adf(spec["nbin_adf"], triples, ordinate=spec["ordinate"], member_by_tag=member)
            d.compute(0, 0)
            out = {}
            for step in range(0, spec["nsteps"] + 1):
                if step:
                    d.step(0, 0, rebuild="auto" if rebuild == "auto" else step % rebuild == 0)
                if step in reads:   # rdf, adf, rdf, adf: the second pair re-reads the state of the first
                    got = [d.rdf_read(), d.adf_read(), d.rdf_read(), d.adf_read()]
                    out[step] = dict(tags=d.tags_local.copy(), x=ctx.md_download(d.nlocal, want=("x",))["x"], got=got)
            return dict(out=out, builds=d.builds, late=d.dangerous)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    types = s.type.copy()      # (by tag: the tags are 1 .. n in order)
    err = dict(rdf_outside=0, adf_outside=0, counts=0, reread=0, ranks=0, edge=0, vacuous=0, not_owned_once=0, late=sum(r["late"] for r in res),
               builds=res[0]["builds"], entries=None, angles=None, most=0)
    exempt = spec["group"]["kind"] in ("tiny", "one type out")
    same = lambda a, b: all(np.array_equal(u, v) for u, v in zip(a, b))
    spec = dict(spec, cutoff_used=cutoff)
    for step in reads:
        x, seen = np.zeros((s.n, 3)), np.zeros(s.n, dtype=int)
        for r in res:
            o = r["out"][step]
            x[o["tags"] - 1] = o["x"]
            seen[o["tags"] - 1] += 1
        err["not_owned_once"] += int(not np.all(seen == 1))
        got = res[0]["out"][step]["got"]
        for r in res[1:]:
            err["ranks"] += int(not all(same(a, b) for a, b in zip(r["out"][step]["got"], got)))
        err["reread"] += int(not (same(got[0], got[2]) and same(got[1], got[3])))
        rref, aref = measure_references(spec, x, types, s.box.h, member)
        (hist, ic, jc, du), (ahist, aic) = got[0], got[1]
        err["rdf_outside"] += _msr_outside(hist, rref)
        err["adf_outside"] += _msr_outside(ahist, aref)
        err["counts"] += int(not (same((ic, jc, du), (rref["icount"], rref["jcount"], rref["dup"])) and np.array_equal(aic, aref["icount"])))
        err["edge"] += rref["n_edge"] + aref["n_edge"] + aref["n_shell_edge"]
        entries, angles = int(rref["hist"].sum()), int(aref["hist"].sum())
        err["entries"] = entries if err["entries"] is None else min(err["entries"], entries)
        err["angles"] = angles if err["angles"] is None else min(err["angles"], angles)
        err["most"] = max(err["most"], aref["max_neighbours"])
    err["vacuous"] = 0 if exempt or (err["entries"] >= MSR_FLOOR and err["angles"] >= MSR_FLOOR) else 1
    return err, dict(rdf_outside=1, adf_outside=1, counts=1, reread=1, ranks=1, edge=MSR_EDGE_LIMIT, vacuous=1, not_owned_once=1, late=1)


def line_measure(spec, err):
    cut = "limit" if spec["cutoff"] is None else f"{spec['cutoff']:.3f}"
    return (f"{spec['id']} size {spec['size']} tilt {spec['tilt'] is not None} relabel {spec['relabel']} free {spec['nonperiodic']} T {spec['temp']} "
            f"drift {spec['drift']} steps {spec['nsteps']} rebuild {spec['rebuild']} read also at {spec['between']} cutoff {cut} "
            f"rcap {spec['rcap']:.2f} fitted {spec['fitted']} seed {spec['seed']} rdf outside {err['rdf_outside']} adf outside {err['adf_outside']} "
            f"counts {err['counts']} reread {err['reread']} ranks {err['ranks']} edge {err['edge']} entries {err['entries']} angles {err['angles']} "
            f"most neighbours {err['most']} vacuous {err['vacuous']} owned once {not err['not_owned_once']} late {err['late']} builds {err['builds']}")


# ------------------------------------------------------------------------------------------------------------ peratom
# compute profile/mdp, msd/mdp and heatflux/mdp (csrc/profile.hip, csrc/msd.hip, csrc/heatflux.hip) on one context per rank,
# against tests/profileref.py, tests/msdref.py and tests/heatfluxref.py on the state gathered by tag from the same run, and
# the heat current of the last read against the oracle's per-atom tallies.  The systems of the measure net (MoS2 replicas,
# the alloy at 5 - 8 cells, all three tilts in some) at 0 K (velocities exactly zero), 300, 1 200 or 2 500 K, some with a
# drift and some of those with 150 A/ps along one axis (atoms cross a face between two reads); 1 - 8 bricks, a free
# dimension in some one-brick alloy cases; no group, a slab, a modulus class, one type left out, 1 - 3 atoms or nobody, on
# group bit 1, 7, 30 or 31; two profile grids of 1 - 3 dimensions in any order, one that fits the workgroup's LDS copy
# (rows * 5 <= 4 096) and, in half of the cases, one that does not (up to PROFILE_MAXBINS rows on one brick, 65 536 on
# several); MDP_MEASURE_GRID unset or 1, 3, 64, and on one brick the
# tables of a knob case once more with the knob unset; msd origins from the current positions or by tag, at step 0 or at
# the read in between (images non-zero by then), read with and without the com shift; reads at step 0, in between and at
# the end, each taken twice, the last step tallying and in half of the cases with its final half left to the first read.
# Every error is a count that must be 0; the reference's own edge atoms (within 1e-9 of a bin edge) are capped at 2 a read.
# The bounds (none measured):
#   profile   counts exact, sums within count 2^-e + 2^-50 sum|t| (profileref.check_sums); rows an edge atom can fall in are
#             bracketed instead (profileref.check_sums_with_edges)
#   xu        |xu - (x + h . image)| <= 8 2^-53 (|x| + sum_k |h_dk image_k|) per component: three fused operations on the
#             device, up to five roundings in msdref.unwrap
#   msd       the sums within MSD_RTOL = 1e-12 (tests/test_gpu_msd_mdp.py) of the sums of their terms' magnitudes; for a
#             read with the com shift the magnitude of a term ((xu - x0) - shift)^2 is (|xu - x0| + |shift|)^2, and the
#             reference subtracts the very shift the device was handed (the shift itself is held to the centre of mass)
#   images    between two reads no atom moves further than half the smallest perpendicular width of the box; the draw keeps
#             1.5 x the speed cap x dt x the steps between two reads below that, so a miscounted image -- a whole box vector --
#             fails whatever the forces did
#   heatflux  the sums within 1e-12 of their terms' magnitudes (tests/test_gpu_heatflux_mdp.py), the count exact, out[7] of
#             all atoms against thermo ke + fsum(eatom); at the last read J and sum W.v within
#             sum|v|_1 (1e-9 + 3e-9 max(1, max|vatom|)) of the oracle's (test_physics_against_the_oracle)
PA_TEMPS = (0, 300, 1200, 2500)
PA_GROUPS = ("none", "slab", "modulus", "one type out", "few", "nobody")
PA_BITS = (1 << 1, 1 << 7, 1 << 30, 1 << 31)
PA_NBIN = (1, 2, 3, 5, 7, 11, 13, 37, 101, 819, 820, 1024)
PA_LDS_ROWS = 819                 # rows * 5 <= 4 096: the largest grid a workgroup keeps in LDS
PA_MAXBINS = 1048576              # PROFILE_MAXBINS of include/mdpair_hip.h (run_peratom asserts it)
PA_BRICK_ROWS = 65536             # ... and the cap on several bricks: the transports carry a table as doubles, a million rows take seconds
PA_FAST = 150                     # A/ps
PA_DT = 0.001
PA_EDGE_LIMIT = 3
PA_RTOL = 1e-12
PA_ORDER = ("profile", "heatflux", "msd")


def _pa_grid(rng, cap, first=None):
    ndim = rng.randint(1, 3)
    dims = rng.sample(range(3), ndim)
    nbins, rows = [], 1
    for k in range(ndim):
        n = rng.choice(first if first and k == 0 else PA_NBIN)
        if rows * n > cap:
            n = max(1, cap // rows)
        nbins.append(n)
        rows *= n
    return tuple(dims), tuple(nbins)


def draw_peratom(rng):
    style = rng.choice(["rebomos", "aeam"])
    sd = rng.randrange(1, 10**6)
    spec = dict(style=style, seed=sd, tilt=None, relabel=None, frac=None, nonperiodic=(0, 0, 0), ntypes=2)
    if style == "rebomos":
        size = (rng.choice([1, 2]), rng.choice([1, 2]), rng.choice([1, 2]))
        spec.update(size=size, n=_rebo_n(size))
    else:
        size = rng.choice([5, 6, 7, 8])
        spec.update(size=size, n=4 * size ** 3, frac=rng.choice([0.05, 0.2, 0.5]))
        if rng.random() < 0.4:   # all three tilts, as draw_measure shears it
            spec["tilt"] = [rng.uniform(-0.12, 0.12) * 4.045 * size for _ in range(3)]
    spec["amp"] = rng.choice([0.02, 0.05, 0.08])
    spec["temp"] = rng.choice(PA_TEMPS)
    spec["drift"] = [rng.choice([-60, -30, 0, 25, 40, 70]) for _ in range(3)] if rng.random() < 0.4 else [0, 0, 0]
    spec["fast"] = (rng.random() < 0.5, rng.randrange(3), rng.choice([-1, 1]))
    spec["nsteps"] = rng.randint(5, 40)
    spec["ranks"] = 1 if rng.random() < 0.5 else rng.choice([2, 3, 4, 8])
    auto, renb = rng.random() < 0.5, rng.choice([3, 5, 8])
    spec["rebuild"] = "auto" if auto and spec["ranks"] == 1 else renb     # (the device's own check serves one brick only)
    free = rng.random() < 0.4, rng.randrange(3)
    if style == "aeam" and spec["ranks"] == 1 and spec["tilt"] is None and free[0]:
        spec["nonperiodic"] = tuple(int(d == free[1]) for d in range(3))
    spec["between"] = rng.randint(1, spec["nsteps"] - 1)
    spec["group"] = dict(kind=rng.choice(PA_GROUPS), axis=rng.randrange(3), lo=rng.uniform(0.0, 0.5), width=rng.uniform(0.3, 0.5),
                         m=rng.choice([2, 3, 5]), r=rng.randrange(2), count=rng.choice([1, 2, 3]), pick=rng.randrange(10**6),
                         type=rng.randint(1, 2), bit=rng.choice(PA_BITS))
    small = _pa_grid(rng, PA_LDS_ROWS)
    cap = PA_MAXBINS if spec["ranks"] == 1 else PA_BRICK_ROWS
    other = _pa_grid(rng, cap, first=(820, 1024)) if rng.random() < 0.5 else _pa_grid(rng, PA_LDS_ROWS)
    spec["grids"] = [small, other] if rng.random() < 0.5 else [other, small]
    spec["env"] = {"MDP_MEASURE_GRID": rng.choice(MSR_GRID)} if rng.random() < 0.5 else {}
    spec["origin"] = dict(mode=rng.choice(["null", "tag"]), at=rng.choice(["start", "between"]))
    if spec["ranks"] > 1:
        spec["origin"]["mode"] = "tag"       # (origins from the current positions are for one rank)
    spec["defer"] = rng.random() < 0.5
    spec["first_read"] = rng.choice(PA_ORDER)
    _pa_fit(spec)
    return spec


def peratom_half_width(box):
    """half the smallest perpendicular width of the box"""
    return 0.5 / float(np.linalg.norm(box.hinv, axis=1).max())


def _pa_fit(spec):
    """no draws: 0 K and a free dimension take the drift out; a drifting case takes PA_FAST along one axis where the rule of
    _cell_velocities still allows a step between two list builds; the steps are cut to what keeps 1.5 x the speed cap x dt x
    the steps between two reads below half the smallest perpendicular width (at least 5 fit every box here); a group of a
    few atoms gets its tags"""
    s = _cell_start(spec)
    if spec["temp"] == 0 or any(spec["nonperiodic"]):
        spec["drift"] = [0, 0, 0]
    spec["fast_on"] = False
    if any(spec["drift"]) and spec["fast"][0]:
        fast = list(spec["drift"])
        fast[spec["fast"][1]] = spec["fast"][2] * PA_FAST
        trial = dict(spec, drift=fast)
        if int(0.3 * MSR_SKIN[spec["style"]] / (_cell_speed_cap(trial, s, _cell_velocities(trial, s)[0]) * PA_DT)) >= 1:
            spec["drift"], spec["fast_on"] = fast, True
    vcap = _cell_speed_cap(spec, s, _cell_velocities(spec, s)[0])
    half = peratom_half_width(s.box)
    most = int(0.98 * half / (1.5 * vcap * PA_DT))      # (2 % for the potentials' masses in place of the placeholders')
    assert most >= 5, (most, half, vcap)
    spec["nsteps"] = min(spec["nsteps"], most)
    spec["between"] = min(spec["between"], spec["nsteps"] - 1)
    spec.update(vcap=vcap, half=half)
    g = spec["group"]
    if g["kind"] == "few":
        g["tags"] = sorted(int(t) + 1 for t in np.random.default_rng(g["pick"]).choice(s.n, g["count"], replace=False))
    spec["heatflux"] = spec["style"] == "rebomos" or spec["ranks"] == 1      # (alloy bricks are refused: tests/test_gpu_heatflux_mdp.py)
    grids = "+".join(".".join(f"{'xyz'[d]}{n}" for d, n in zip(*gr)) for gr in spec["grids"])
    bit = g["bit"].bit_length() - 1
    spec["id"] = (f"{spec['style']}-n{spec['n']}-ranks{spec['ranks']}-T{spec['temp']}-{g['kind'].replace(' ', '')}-bit{bit}-{grids}-"
                  f"grid{spec['env'].get('MDP_MEASURE_GRID', 'unset')}-origin{spec['origin']['mode']}at{spec['origin']['at']}")


def peratom_member(spec, s):
    """the member table of the case by tag (row t - 1), or None for no group; s: the start system"""
    g = spec["group"]
    if g["kind"] == "nobody":
        return np.zeros(s.n, dtype=bool)
    if g["kind"] == "few":
        m = np.zeros(s.n, dtype=bool)
        m[np.array(g["tags"]) - 1] = True
        return m
    return group_member(spec, s)


def peratom_rows(grid):
    return int(np.prod(grid[1]))


def _pa_oracle_currents(spec, s, x, v, member):
    """heatfluxref.sums with the ORACLE's per-atom tallies on positions by tag, and the scale of its vatom.  A free dimension:
    the box grows by 30 A either way in it, so that no periodic image comes within reach"""
    import dataclasses
    import heatfluxref
    import mdref
    R = _res()
    box = s.box
    if any(spec["nonperiodic"]):
        free = np.array(spec["nonperiodic"]) == 1
        lam = box.x2lamda(x)
        assert not box.tilt.any() and float((np.maximum(-lam, lam - 1.0) * box.prd)[:, free].max()) < 15.0    # no atom far outside
        pad = 30.0 * free
        box = S.Box(box.lo - pad, box.prd + 2.0 * pad, box.tilt.copy())
    s2 = dataclasses.replace(s, box=box, x=S.wrap(box, x))
    eng = mdref.RebomosCPU(R["orc"], R["P"], s2) if spec["style"] == "rebomos" else mdref.AeamCPU(R["orc"], R["T"], s2)
    o = eng.compute(s2.x)
    n = s.n
    ea, va = o["eatom"][:n].copy(), o["vatom"][:n].copy()
    np.add.at(ea, eng.owner, o["eatom"][n:])         # the oracle's ghost shares onto their owners
    np.add.at(va, eng.owner, o["vatom"][n:])
    return heatfluxref.sums(s.mass[s.type], v, ea, va, S.MVV2E, member=member), max(1.0, float(np.abs(va).max()))


def run_peratom(spec):
    import math
    import heatfluxref
    import msdref
    import profileref
    from lammps_plugins_amd.host import capi, resident
    assert capi.PROFILE_MAXBINS == PA_MAXBINS and capi.PROFILE_W == profileref.W
    s = _cell_start(spec)
    tabs, cutghost = _cell_potential(spec, s)
    n, world, nsteps, hf = s.n, spec["ranks"], spec["nsteps"], spec["heatflux"]
    member = peratom_member(spec, s)
    bit = spec["group"]["bit"] if member is not None else 0
    gbit = bit - (1 << 32) if bit >= (1 << 31) else bit             # the C int with that bit
    mask = np.ones(n + 1, dtype=np.uint32)
    if member is not None:
        mask[1:] |= np.where(member, np.uint32(bit), np.uint32(0))
    mask = mask.view(np.int32)
    sel = np.ones(n, dtype=bool) if member is None else member
    mass = s.mass[s.type]
    v0, safe = _cell_velocities(spec, s)
    rebuild = spec["rebuild"] if spec["rebuild"] == "auto" else min(spec["rebuild"], safe)
    reads = sorted({0, spec["between"], nsteps})
    origin_at = 0 if spec["origin"]["at"] == "start" else spec["between"]
    knob = "MDP_MEASURE_GRID" in spec["env"] and world == 1
    plain_env = {k: v for k, v in spec["env"].items() if k != "MDP_MEASURE_GRID"}
    k0 = PA_ORDER.index(spec["first_read"])
    order = PA_ORDER[k0:] + PA_ORDER[:k0]
    by_tag = lambda tags, a: _by_tag_rows(n, tags, a)

    def rank_fn(r, make_tr):
        ctx, d = _cell_domain(spec, s, tabs, cutghost, v0, make_tr)
        try:
            if member is not None:
                d.set_group(mask, 0)
            d.track_images()
            tally = (3, 5) if hf else (0, 0)
            d.compute(*tally)
            out, msd = {}, {}
            for step in range(0, nsteps + 1):
                if step:
                    last = step == nsteps
                    d.step(*((3, 5) if last or (hf and step in reads) else (0, 0)),
                           rebuild="auto" if rebuild == "auto" else step % rebuild == 0, defer_final=last and spec["defer"])
                    if last and spec["defer"]:
                        d._final_pending = False      # the library holds the half: the first read that needs velocities completes it
                if step not in reads:
                    continue
                o = dict(prof=[], plain=[])
                for what in order:
                    if what == "profile":
                        for dims, nbins in spec["grids"]:
                            d.profile(dims, nbins, group_bit=gbit)
                            o["prof"].append((d.profile_read(), d.profile_read()))
                            if knob:
                                with knobs(plain_env):
                                    o["plain"].append(d.profile_read())
                    elif what == "heatflux" and hf:
                        o["hf"] = [d._group_sum(ctx.heatflux_sums(gbit)) for _ in range(2)]
                        o["hf_all"] = d._group_sum(ctx.heatflux_sums(0))
                    elif what == "msd":
                        tags, xu = d.tags_local, d.unwrapped_local()
                        if step == origin_at:
                            x0 = np.zeros((n, 3))
                            x0[tags - 1] = xu
                            if world > 1:
                                x0 = d._group_sum(x0.ravel()).reshape(n, 3)
                            ctx.msd_setup(n, None if spec["origin"]["mode"] == "null" else x0, gbit)
                            msd.update(x0=x0, cm0=msdref.centre_of_mass(x0[sel], mass[sel]) if sel.any() else np.zeros(3))
                        if msd:
                            o["msd"] = [d._group_sum(ctx.msd_sums()) for _ in range(2)]
                            o["x0"] = msd["x0"]
                            if o["msd"][0][7] > 0.0:
                                o["shift"] = o["msd"][0][4:7] / o["msd"][0][7] - msd["cm0"]
                                o["msd_com"] = d._group_sum(ctx.msd_sums(o["shift"]))
                tallied = hf
                got = ctx.md_download(d.nlocal, want=("x", "v", "eatom") if tallied else ("x", "v"))
                o.update(tags=d.tags_local.copy(), x=got["x"], v=got["v"], image=d.images_local(), xu=d.unwrapped_local())
                if tallied:
                    o.update(eatom=got["eatom"], vatom=ctx.md_download_vatom(d.nlocal), ke=d.thermo()["ke"])
                out[step] = o
            return dict(out=out, builds=d.builds, late=d.dangerous)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    err = dict(reread=0, ranks=0, not_owned_once=0, exponents=0, profile=0, knob=0, edge=0, xu_outside=0, msd_outside=0, msd_count=0,
               jumped=0, premise=0, hf_outside=0, hf_count=0, hf_energy=0, hf_physics=0, late=sum(r["late"] for r in res),
               builds=res[0]["builds"], xu=0.0, msd=0.0, hf=0.0, prof=0.0, physics=0.0, failed=[])
    same = lambda a, b: all(np.array_equal(u, w) for u, w in zip(a, b))
    per = tuple(bool(p) for p in _cell_periodic(spec))
    vcap = _cell_speed_cap(spec, s, v0)
    half = peratom_half_width(s.box)
    before = None
    for step in reads:
        g = dict(seen=np.zeros(n, dtype=int))
        for r in res:
            o = r["out"][step]
            g["seen"][o["tags"] - 1] += 1
            for key in ("x", "v", "image", "xu", "eatom", "vatom"):
                if key in o:
                    a = o[key] if o[key].ndim > 1 else o[key][:, None]
                    g.setdefault(key, np.zeros((n, a.shape[1]), dtype=a.dtype))[o["tags"] - 1] = a
        err["not_owned_once"] += int(not np.all(g["seen"] == 1))
        o = res[0]["out"][step]
        # ---- every compute: two reads of one state identical, every rank reads the same
        err["reread"] += sum(int(not same(a, b)) for a, b in o["prof"])
        for key in ("hf", "msd"):
            if key in o:
                err["reread"] += int(o[key][0].tobytes() != o[key][1].tobytes())
        for r in res[1:]:
            q = r["out"][step]
            err["ranks"] += sum(int(not same(a[0], b[0])) for a, b in zip(q["prof"], o["prof"]))
            err["ranks"] += sum(int(not np.array_equal(q[key], o[key])) for key in ("hf", "hf_all", "msd", "msd_com") if key in o)
        # ---- profile
        lam = s.box.x2lamda(g["x"])
        for k, (dims, nbins) in enumerate(spec["grids"]):
            count, sums, ex = o["prof"][k][0]
            ref = profileref.table(lam, per, dims, nbins, mass, g["v"], exponents=ex, member=member, natoms_total=n)
            err["exponents"] += int(ex.tolist() != [profileref.exponent(q, n) for q in ref["rng"]])
            try:
                worst, n_edge = profileref.check_sums_with_edges(count, sums, ex, ref, profileref.edges(lam, per, dims, nbins, member))
                err["prof"], err["edge"] = max(err["prof"], worst), max(err["edge"], n_edge)
            except AssertionError as e:
                err["profile"] += 1
                err["failed"].append(f"profile step {step} grid {k}: {str(e)[:200]}")
            if knob:
                err["knob"] += int(not same(o["plain"][k], o["prof"][k][0]))
        # ---- msd: the unwrapped positions, the sums, the images
        want = msdref.unwrap(s.box, g["x"], g["image"])
        bound = 8.0 * 2.0 ** -53 * (np.abs(g["x"]) + S.mul_upper(np.abs(g["image"]).astype(np.float64), np.abs(s.box.h)))
        dxu = np.abs(g["xu"] - want)
        err["xu_outside"] += int((dxu > bound).sum())
        err["xu"] = max(err["xu"], float(dxu.max()))
        if "msd" in o:
            got, x0, nsel = o["msd"][0], o["x0"], int(sel.sum())
            err["msd_count"] += int(got[3] != nsel)
            if nsel == 0:
                err["msd_outside"] += int(np.any(got != 0.0))
            else:
                xs, os_, ms = g["xu"][sel], x0[sel], mass[sel]
                means = msdref.msd_values(g["xu"], x0, sel=sel)[:3]          # (terms of one sign: the sum is its own magnitude)
                pairs = list(zip(got[:3] / got[3], means, means))
                cm, mtot = msdref.centre_of_mass(xs, ms), math.fsum(ms)
                pairs += [(got[4 + c] / got[7], cm[c], math.fsum(np.abs(ms * xs[:, c])) / mtot) for c in range(3)]
                pairs.append((got[7], mtot, mtot))
                if "msd_com" in o:
                    dd = (xs - os_) - o["shift"]
                    mg = np.abs(xs - os_) + np.abs(o["shift"])
                    pairs += [(o["msd_com"][c] / o["msd_com"][3], math.fsum(dd[:, c] * dd[:, c]) / nsel, math.fsum(mg[:, c] * mg[:, c]) / nsel)
                              for c in range(3)]
                    err["msd_count"] += int(o["msd_com"][3] != nsel)
                for a, b, m in pairs:
                    err["msd_outside"] += int(not abs(a - b) <= PA_RTOL * m)
                    if m > 0.0:
                        err["msd"] = max(err["msd"], abs(a - b) / m)
        if before is not None:
            gap = step - before[0]
            err["premise"] += int(not 1.5 * vcap * PA_DT * gap < half)
            err["jumped"] += int((np.sqrt(((g["xu"] - before[1]) ** 2).sum(axis=1)) > half).sum())
        before = (step, g["xu"])
        # ---- heatflux
        if "hf" in o:
            ref = heatfluxref.sums(mass, g["v"], g["eatom"][:, 0], g["vatom"], S.MVV2E, member=member)
            got = o["hf"][0]
            err["hf_count"] += int(got[6] != sel.sum())
            err["hf_outside"] += int((~(np.abs(got - ref["sums"]) <= PA_RTOL * ref["mag"])).sum())
            ok = ref["mag"] > 0.0
            if ok.any():
                err["hf"] = max(err["hf"], float((np.abs(got - ref["sums"])[ok] / ref["mag"][ok]).max()))
            everyone = heatfluxref.sums(mass, g["v"], g["eatom"][:, 0], g["vatom"], S.MVV2E)
            err["hf_energy"] += int(not abs(o["hf_all"][7] - (o["ke"] + math.fsum(g["eatom"][:, 0]))) <= PA_RTOL * everyone["mag"][7])
            err["hf_energy"] += int(o["hf_all"][6] != n)
            if step == nsteps:
                oref, scale = _pa_oracle_currents(spec, s, g["x"], g["v"], member)
                bound = float(np.abs(g["v"][sel]).sum()) * (1e-9 + 3e-9 * scale)
                vec = np.concatenate([got[0:3] + got[3:6], got[0:3]])
                diff = np.concatenate([np.abs(vec - oref["vector"]), np.abs(got[3:6] - oref["sums"][3:6])])
                err["hf_physics"] += int((~(diff <= bound)).sum())
                if bound > 0.0:
                    err["physics"] = float(diff.max() / bound)
    lim = dict.fromkeys(("reread", "ranks", "not_owned_once", "exponents", "profile", "knob", "xu_outside", "msd_outside", "msd_count", "jumped",
                         "premise", "hf_outside", "hf_count", "hf_energy", "hf_physics", "late"), 1)
    lim["edge"] = PA_EDGE_LIMIT
    return err, lim


def _by_tag_rows(n, tags, a):
    out = np.zeros((n,) + a.shape[1:], dtype=a.dtype)
    out[tags - 1] = a
    return out


def line_peratom(spec, err):
    g = spec["group"]
    return (f"{spec['id']} size {spec['size']} tilt {spec['tilt'] is not None} free {spec['nonperiodic']} drift {spec['drift']} steps {spec['nsteps']} "
            f"rebuild {spec['rebuild']} read also at {spec['between']} defer {spec['defer']} first {spec['first_read']} heatflux {spec['heatflux']} "
            f"seed {spec['seed']} reread {err['reread']} ranks {err['ranks']} exponents {err['exponents']} profile {err['profile']} knob {err['knob']} "
            f"edge atoms {err['edge']} xu outside {err['xu_outside']} msd outside {err['msd_outside']} count {err['msd_count']} jumped {err['jumped']} "
            f"premise {err['premise']} heatflux outside {err['hf_outside']} count {err['hf_count']} energy {err['hf_energy']} physics {err['hf_physics']} "
            f"owned once {not err['not_owned_once']} late {err['late']} builds {err['builds']} worst: |xu - ref| {err['xu']:.2e} A, msd {err['msd']:.2e}, "
            f"heatflux / mag {err['hf']:.2e}, profile / bound {err['prof']:.3f}, J / physics bound {err['physics']:.2e}"
            + ("".join("  " + f for f in err["failed"])))


# ---------------------------------------------------------------------------------------------------------- structure
# compute coord/atom/mdp, centro/atom/mdp and cna/atom/mdp (csrc/coord.hip, csrc/centro.hip, csrc/cna.hip on the walk of
# csrc/measure_walk.h behind csrc/measure_bin.hip), all three set up on one context per rank, against tests/structref.py and
# tests/cnaref.py on positions merged by tag from the same state.  The thermal cells of the peratom net (MoS2 replicas, the
# alloy at 5 - 8 cells, all three tilts in some, relabelled to 3 - 12 types in half: coord's columns), 0 - 2 500 K, some with
# a drift, 1 - 8 bricks, a free dimension in some one-brick alloy cases; in a quarter of the cases a constructed cell of
# cnaref in their place (the close-packed stack, bcc, the 13-atom icosahedron; jitter 0.02 - 0.05 A), read with no steps, on
# 1, 2 or 4 bricks: the only hcp, bcc and icosahedral centres here.  One group for the three computes: none, a slab, a
# modulus class, one type left out, 1 - 3 atoms or nobody, on bit 1, 7, 30 or 31.  coord: 1 - 32 columns of random type
# ranges, the cutoff just above the first shell (where bin_grid widens its cells), anywhere up to the radius cap, or the cap;
# centro: N of 2 - 64 (17 - 88 KB of LDS a workgroup), the cutoff the shell's limit or drawn; cna: the cutoff around the
# canonical one of the lattice (0.80 - 0.92 a for fcc and hcp, which brackets 0.8536 a, and in 3 of 10 sets 0.96 - 1.04 a,
# over the second shell: structure_cna_range; 1.15 - 1.26 a for bcc; 0.9 - 1.1 x 1.35 r for the icosahedron; 2.6 - 3.6 A
# for MoS2).  The radius cap: no centre has more than 100 atoms
# inside it at the start (the short list holds 128, and a centro read over it is refused by design); where the shell's limit
# lies above it (MoS2), "the limit" is the cap (spec: centro_capped).  MDP_MEASURE_GRID unset or 1, 3, 64.  Reads at step 0,
# in between and at the end, each taken twice (coord, centro, cna, and the three again); then either a second parameter set
# on the same contexts (other cutoffs: other grids and bin buffers; other columns: val regrows; another N: another LDS
# size) or *_off and the first set again, which must return the last read bit for bit.
# Every error is a count that must be 0.  The bounds (none measured):
#   coord    count_sure <= device <= count_sure + edge in every cell (structref.coord: equality but for pairs within 1e-9 of
#            the cutoff), integers, rows outside the group exactly 0
#   centro   |device - reference| <= structref.centro_bound(N, cutoff, Lmax) = 64 eps N cutoff Lmax (derived there from the
#            roundings of x + shift and of the differences) for every atom that is not ambiguous; exactly 0 with fewer than N
#            inside; the sum of centro_info()["few"] equal to the reference's count to within the ambiguous atoms; no refusal
#   cna      the pattern equal for every atom that is not ambiguous; the census the histogram of the values handed out;
#            cna_info()["over"] the reference's count of centres with more than 16 neighbours to within the ambiguous atoms
# A condition of the case: the reference's own ambiguous atoms and edge pairs are at most 2 per read and compute, the fixed
# tests' cap (tests/test_net_draws.py checks it on the start positions, with the floors: unless the case is about a group of
# 0 - 3 atoms or the icosahedron, 100 centres have N inside and 100 a non-zero coordination number).
# Measured on an MI355X, the 16 suite cases (seed 1018) and 200 cases at seed 7 through profiles/structure_fuzz.py: 16 of 16
# and 200 of 200 inside every bound.  Worst centro error 0.001 and 0.002 of structref.centro_bound (as printed, to three
# decimals); the largest `inside` of any atom 104 and 110 (the draw's cap is 100 at the start, the list holds 128; no read
# was refused); the largest `few` of a read 0 and 1 918, the largest `over` 960 and 1 743; no edge pair or ambiguous atom in
# any read (cap 2), no late check.  The suite's cases take 14.5 s of calls, the longest 2.4 s; of the 200 the longest took
# 17.3 s (2 304 MoS2 atoms, N = 64, the knob at 1: one workgroup ranks 2 016 pair values for every centre), the next 4.7 s.
# The net found no bug in the library.
STR_CELLS = ("stack", "bcc", "icosahedron")
STR_CELL_N = {"stack": 960, "bcc": 1024, "icosahedron": 13}
STR_COLS = (1, 2, 3, 8, 17, 32)
STR_N = (2, 4, 6, 8, 12, 14, 16, 32, 64)
STR_CUTOFFS = ("shell", "uniform", "cap")
STR_FLOOR = 100                   # centres with N inside, and with a non-zero coordination number, at the start
STR_EDGE_LIMIT = 3                # the reference's ambiguous atoms and edge pairs of a read and compute: at most 2
_STR_DRAWN = {}


def structure_cna_range(spec, across=False):
    """the interval the cna cutoff of a case is drawn from.  across (fcc-like cells only): over the second shell, 0.96 - 1.04 a,
    where the jitter of the start positions alone leaves 12 - 18 neighbours -- below 0.92 a no start position has a thirteenth
    (the second shell lies 0.32 A further out, the jitter moves a pair by 0.16 A at most, and a shear only lengthens the cube
    axes), and tests/test_net_draws.py asks the start positions for 13, 15, 16 and 17"""
    import cnaref
    if spec["cell"] == "bcc":
        return 1.15 * cnaref.A_BCC, 1.26 * cnaref.A_BCC
    if spec["cell"] == "icosahedron":
        return 0.9 * cnaref.RC_ICO, 1.1 * cnaref.RC_ICO
    if spec["style"] == "rebomos":
        return 2.6, 3.6
    return (0.96 * cnaref.A_FCC, 1.04 * cnaref.A_FCC) if across else (0.80 * cnaref.A_FCC, 0.92 * cnaref.A_FCC)


def _str_params(rng, nt):
    """the draws of one parameter set; the radii are fractions here (_str_fit)"""
    cols = [_msr_range(rng, nt) for _ in range(rng.choice(STR_COLS))]
    return dict(cols=cols, coord_kind=rng.choice(STR_CUTOFFS), coord_shell=rng.uniform(1.02, 1.15), coord_u=rng.random(),
                nnn=rng.choice(STR_N), centro_limit=rng.random() < 0.5, centro_u=rng.random(), cna_u=rng.random(), cna_across=rng.random() < 0.3)


def draw_structure(rng):
    import copy
    key = rng.getstate()
    if key in _STR_DRAWN:     # (the geometry of _str_fit costs seconds; the draw is a function of the generator's state)
        spec, after = _STR_DRAWN[key]
        rng.setstate(after)
        return copy.deepcopy(spec)
    spec = _str_random(rng)
    _str_fit(spec)
    _STR_DRAWN[key] = (copy.deepcopy(spec), rng.getstate())
    return spec


def _str_random(rng):
    """the draws of a case; _str_fit then makes radii of the fractions and meets the floors on the start positions without drawing"""
    sd = rng.randrange(1, 10**6)
    spec = dict(seed=sd, cell=None, size=None, tilt=None, relabel=None, frac=None, nonperiodic=(0, 0, 0), ntypes=2, temp=0, drift=[0, 0, 0],
                nsteps=0, between=0, rebuild="auto")
    if rng.random() < 0.25:       # a constructed cell: one type of the alloy's, read after the setup compute
        cell = rng.choice(STR_CELLS)
        spec.update(style="aeam", cell=cell, n=STR_CELL_N[cell], amp=rng.uniform(0.02, 0.05))
        ranks = rng.choice([1, 2, 4])
        spec["ranks"] = 1 if cell == "icosahedron" else ranks
    else:
        style = rng.choice(["rebomos", "aeam"])
        spec["style"] = style
        if style == "rebomos":
            size = (rng.choice([1, 2]), rng.choice([1, 2]), rng.choice([1, 2]))
            spec.update(size=size, n=_rebo_n(size))
        else:
            size = rng.choice([5, 6, 7, 8])
            spec.update(size=size, n=4 * size ** 3, frac=rng.choice([0.05, 0.2, 0.5]))
            if rng.random() < 0.4:   # all three tilts, as draw_measure shears it
                spec["tilt"] = [rng.uniform(-0.12, 0.12) * 4.045 * size for _ in range(3)]
            if rng.random() < 0.5:   # relabelled to 3 - 12 types, as draw_measure relabels it
                spec["relabel"] = rng.choice([(2, 1), (3, 2), (4, 2), (5, 3), (7, 5), (1, 3), (6, 2)])
                spec["ntypes"] = sum(spec["relabel"])
        spec["amp"] = rng.choice([0.02, 0.05, 0.08])
        spec["temp"] = rng.choice(PA_TEMPS)
        spec["drift"] = [rng.choice([-60, -30, 0, 25, 40, 70]) for _ in range(3)] if rng.random() < 0.4 else [0, 0, 0]
        spec["nsteps"] = rng.randint(5, 40)
        spec["ranks"] = 1 if rng.random() < 0.5 else rng.choice([2, 3, 4, 8])
        auto, renb = rng.random() < 0.5, rng.choice([3, 5, 8])
        spec["rebuild"] = "auto" if auto and spec["ranks"] == 1 else renb     # (the device's own check serves one brick only)
        free = rng.random() < 0.4, rng.randrange(3)
        if style == "aeam" and spec["ranks"] == 1 and spec["tilt"] is None and free[0]:
            spec["nonperiodic"] = tuple(int(d == free[1]) for d in range(3))
        spec["between"] = rng.randint(1, spec["nsteps"] - 1)
    nt = spec["ntypes"]
    spec["group"] = dict(kind=rng.choice(PA_GROUPS), axis=rng.randrange(3), lo=rng.uniform(0.0, 0.5), width=rng.uniform(0.3, 0.5),
                         m=rng.choice([2, 3, 5]), r=rng.randrange(2), count=rng.choice([1, 2, 3]), pick=rng.randrange(10**6),
                         type=rng.randint(1, nt), bit=rng.choice(PA_BITS))
    spec["first"] = _str_params(rng, nt)
    spec["second"] = _str_params(rng, nt) if rng.random() < 0.5 else None      # None: *_off and the first set again
    spec["env"] = {"MDP_MEASURE_GRID": rng.choice(MSR_GRID)} if rng.random() < 0.5 else {}
    return spec


def structure_sets(spec):
    """the parameter sets of a case: one or two"""
    return [spec["first"]] + ([spec["second"]] if spec["second"] is not None else [])


def structure_start_counts(spec, p, s, member, pairs):
    """(centres with N inside the centro cutoff, centres with a non-zero coordination number in some column) of the set p on
    the start positions, from the pair list (i, j, r): exact counts"""
    pi, pj, pr = pairs
    mem = np.ones(s.n, dtype=bool) if member is None else member
    ccut = MSR_LIMIT[spec["style"]] if p["centro_cutoff"] is None else p["centro_cutoff"]
    inside = np.bincount(pi[pr < ccut], minlength=s.n)
    near, tj = pr < p["coord_cutoff"], s.type[pj]
    some = np.zeros(s.n, dtype=bool)
    for lo, hi in p["cols"]:
        some |= np.bincount(pi[near & _msr_in(tj, lo, hi)], minlength=s.n) > 0
    return int((mem & (inside >= p["nnn"])).sum()), int((mem & some).sum())


def _str_fit(spec):
    """no draws: 0 K and a free dimension take the drift out; a group of a few atoms gets its tags; the fractions of the sets
    become radii -- between 1.02 first shells and the radius cap of _cell_rcap --; and a case that is not exempt (a group of
    0 - 3 atoms, the icosahedron) meets STR_FLOOR on the start positions with each set: column 1 over all types; then centro's
    cutoff at the limit (the cap); then N lowered; then no group (and N lowered once more)"""
    style, nt = spec["style"], spec["ntypes"]
    first, limit = MSR_FIRST[style], MSR_LIMIT[style]
    if spec["temp"] == 0 or any(spec["nonperiodic"]):
        spec["drift"] = [0, 0, 0]
    s = _cell_start(spec)
    pairs = _msr_pairs(s, spec, limit)
    rcap = _cell_rcap(s, pairs, limit)
    binds = bool(rcap < 0.999 * limit)           # some centre has more than MSR_NEIGH atoms inside the limit
    spec["rcap"] = float(rcap)
    g = spec["group"]
    if g["kind"] == "few":
        g["tags"] = sorted(int(t) + 1 for t in np.random.default_rng(g["pick"]).choice(s.n, g["count"], replace=False))
    exempt = g["kind"] in ("few", "nobody") or spec["cell"] == "icosahedron"
    for p in structure_sets(spec):
        at_cap = lambda: (float(rcap), True) if binds else (None, False)
        low = min(1.02 * first, rcap)
        p["coord_cutoff"] = float({"shell": min(p["coord_shell"] * first, rcap), "uniform": low + p["coord_u"] * (rcap - low), "cap": rcap}[p["coord_kind"]])
        p["centro_cutoff"], p["centro_capped"] = at_cap() if p["centro_limit"] else (float(low + p["centro_u"] * (rcap - low)), False)
        lo, hi = structure_cna_range(spec, p["cna_across"])
        p["cna_cutoff"] = float(lo + p["cna_u"] * (hi - lo))
        p["fitted"] = []
        if exempt:
            continue
        met = lambda: structure_start_counts(spec, p, s, peratom_member(spec, s), pairs)

        def lower():      # (to the largest N that meets the floor; if none does, N stays)
            drawn = p["nnn"]
            for nnn in reversed([k for k in STR_N if k < drawn]):
                p["nnn"] = nnn
                if met()[0] >= STR_FLOOR:
                    p["fitted"].append("N lowered")
                    return
            p["nnn"] = drawn
        if met()[1] < STR_FLOOR:
            p["cols"][0] = (1, nt)
            p["fitted"].append("all types")
        if met()[0] < STR_FLOOR and not p["centro_limit"]:
            p["centro_cutoff"], p["centro_capped"] = at_cap()
            p["centro_limit"] = True
            p["fitted"].append("centro at the limit")
        if met()[0] < STR_FLOOR:
            lower()
        if min(met()) < STR_FLOOR:
            g["kind"] = "none"
            p["fitted"].append("no group")
            if met()[0] < STR_FLOOR:
                lower()
    p = spec["first"]
    what = spec["cell"] or style
    spec["id"] = (f"{what}-n{spec['n']}-types{nt}-ranks{spec['ranks']}-T{spec['temp']}-{g['kind'].replace(' ', '')}-bit{g['bit'].bit_length() - 1}-"
                  f"col{len(p['cols'])}-N{p['nnn']}-grid{spec['env'].get('MDP_MEASURE_GRID', 'unset')}-{'second' if spec['second'] else 'again'}")


def structure_references(spec, p, x, types, h, member):
    """structref.coord, structref.centro and cnaref.cna of the set p on positions and types by tag, and centro's cutoff"""
    import cnaref
    import structref
    per = _cell_periodic(spec)
    ccut = MSR_LIMIT[spec["style"]] if p["centro_cutoff"] is None else p["centro_cutoff"]
    return (structref.coord(x, types, h, per, p["coord_cutoff"], p["cols"], member), structref.centro(x, h, per, p["nnn"], ccut, member),
            cnaref.cna(x, h, per, p["cna_cutoff"], member), ccut)


def run_structure(spec):
    import structref
    from lammps_plugins_amd.host import capi, resident
    s = _cell_start(spec)
    tabs, cutghost = _cell_potential(spec, s)
    n, world, nsteps = s.n, spec["ranks"], spec["nsteps"]
    member = peratom_member(spec, s)
    bit = spec["group"]["bit"] if member is not None else 0
    gbit = bit - (1 << 32) if bit >= (1 << 31) else bit             # the C int with that bit
    mask = np.ones(n + 1, dtype=np.uint32)
    if member is not None:
        mask[1:] |= np.where(member, np.uint32(bit), np.uint32(0))
    mask = mask.view(np.int32)
    sel = np.ones(n, dtype=bool) if member is None else member
    v0, rebuild = None, "auto"
    if spec["cell"] is None:
        v0, safe = _cell_velocities(spec, s)
        rebuild = spec["rebuild"] if spec["rebuild"] == "auto" else min(spec["rebuild"], safe)
    reads = sorted({0, spec["between"], nsteps})
    lmax = float(np.linalg.norm(s.box.h, axis=0).max())             # (test_gpu_struct_mdp._lmax)

    def setup(d, p):
        d.coord(p["coord_cutoff"], p["cols"], group_bit=gbit)
        d.centro(p["nnn"], p["centro_cutoff"], group_bit=gbit)
        d.cna(p["cna_cutoff"], group_bit=gbit)

    def read(ctx, d):
        """coord, centro, cna and the three again: the second round re-reads the state of the first"""
        o = dict(tags=d.tags_local.copy(), x=ctx.md_download(d.nlocal, want=("x",))["x"], coord=[], centro=[], cna=[], refused="")
        for _ in range(2):
            o["coord"].append(d.coord_read())
            try:
                o["centro"].append(d.centro_read() + (np.array([ctx.centro_info()["few"]]),))
            except capi.MdpError as e:
                o["refused"] = str(e)[-200:]
            o["cna"].append(d.cna_read() + (ctx.cna_counts(), np.array([ctx.cna_info()["over"]])))
        return o

    def rank_fn(r, make_tr):
        ctx, d = _cell_domain(spec, s, tabs, cutghost, v0, make_tr)
        try:
            if member is not None:
                d.set_group(mask, 0)
            setup(d, spec["first"])
            d.compute(0, 0)
            out = {}
            for step in range(0, nsteps + 1):
                if step:
                    d.step(0, 0, rebuild="auto" if rebuild == "auto" else step % rebuild == 0)
                if step in reads:
                    out[step] = read(ctx, d)
            if spec["second"] is not None:
                setup(d, spec["second"])
            else:
                d.coord_off(), d.centro_off(), d.cna_off()
                setup(d, spec["first"])
            out["again"] = read(ctx, d)
            return dict(out=out, builds=d.builds, late=d.dangerous)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    types = s.type.copy()      # (by tag: the tags are 1 .. n in order)
    err = dict(reread=0, tags=0, not_owned_once=0, outside=0, coord=0, integers=0, centro=0, short=0, few=0, refused=0, cna=0, census=0, over=0,
               fresh=0, edge=0, late=sum(r["late"] for r in res), builds=res[0]["builds"], worst=0.0, most=0, most_few=0, most_over=0,
               centres=None, failed=[])
    same = lambda a, b: len(a) == len(b) and all(u.tobytes() == w.tobytes() for u, w in zip(a, b))
    last = None
    for state in reads + ["again"]:
        p = spec["second"] if state == "again" and spec["second"] is not None else spec["first"]
        ncol = len(p["cols"])
        x, seen = np.zeros((n, 3)), np.zeros(n, dtype=int)
        co, ce, cn = np.zeros((n, ncol)), np.zeros(n), np.zeros(n)
        few, over, census, refused = 0, 0, np.zeros(6, dtype=np.int64), False
        for r in res:
            o = r["out"][state]
            tags = o["tags"]
            x[tags - 1] = o["x"]
            seen[tags - 1] += 1
            refused |= bool(o["refused"]) or len(o["centro"]) != 2
            if o["refused"]:
                err["failed"].append(f"read {state}: {o['refused']}")
            for key in ("coord", "centro", "cna"):
                got = o[key]
                if len(got) == 2:
                    err["reread"] += int(not same(got[0], got[1]))
                err["tags"] += sum(int(not np.array_equal(q[0], tags)) for q in got)
            co[tags - 1] = o["coord"][0][1]
            cn[tags - 1] = o["cna"][0][1]
            census += o["cna"][0][2]
            over += int(o["cna"][0][3][0])
            if not refused:
                ce[tags - 1] = o["centro"][0][1]
                few += int(o["centro"][0][2][0])
        err["not_owned_once"] += int(not np.all(seen == 1))
        err["refused"] += int(refused)
        now = (co, ce, cn, census, few, over)
        if state == "again" and spec["second"] is None:     # the fresh setup of the same set on the same state: the last read again
            err["fresh"] += int(not (same(now[:4], last[:4]) and now[4:] == last[4:]))
            continue
        last = now
        cref, zref, aref, ccut = structure_references(spec, p, x, types, s.box.h, member)
        err["outside"] += int((co[~sel] != 0.0).sum() + (ce[~sel] != 0.0).sum() + (cn[~sel] != 0.0).sum())
        # ---- coord
        err["integers"] += int((co != np.rint(co)).sum())
        err["coord"] += int(((co < cref["count_sure"]) | (co > cref["count_sure"] + cref["edge"])).sum())
        # ---- centro
        amb = zref["ambiguous"]
        namb = int(amb.sum())
        short = sel & (zref["inside"] < p["nnn"])
        if not refused:
            bound = structref.centro_bound(p["nnn"], ccut, lmax)
            dz = np.abs(ce - zref["value"])
            err["centro"] += int((~(dz <= bound) & ~amb).sum())
            err["short"] += int((short & ~amb & (ce != 0.0)).sum())
            err["few"] += int(abs(few - int(short.sum())) > namb)
            if (~amb).any():
                err["worst"] = max(err["worst"], float(dz[~amb].max() / bound))
        # ---- cna
        camb = aref["ambiguous"]
        err["cna"] += int(((cn != aref["pattern"]) & ~camb).sum())
        err["census"] += int(not (np.array_equal(census, np.bincount(cn[sel].astype(np.int64), minlength=6)[:6]) and census[0] == 0))
        many = int((sel & (aref["neighbours"] > 16)).sum())
        err["over"] += int(abs(over - many) > int(camb.sum()))
        err["edge"] = max(err["edge"], cref["n_edge"], namb, int(camb.sum()))
        full = int((sel & (zref["inside"] >= p["nnn"])).sum())
        err["centres"] = full if err["centres"] is None else min(err["centres"], full)
        err.update(most=max(err["most"], int(zref["inside"].max(initial=0))), most_few=max(err["most_few"], few), most_over=max(err["most_over"], over))
    lim = dict.fromkeys(("reread", "tags", "not_owned_once", "outside", "coord", "integers", "centro", "short", "few", "refused", "cna", "census",
                         "over", "fresh", "late"), 1)
    lim["edge"] = STR_EDGE_LIMIT
    return err, lim


def line_structure(spec, err):
    def text(p):
        cut = "limit" if p["centro_cutoff"] is None else f"{p['centro_cutoff']:.3f}" + (" (the limit, capped)" if p["centro_capped"] else "")
        return (f"coord {len(p['cols'])} columns inside {p['coord_cutoff']:.3f} ({p['coord_kind']}), centro N {p['nnn']} inside {cut}, "
                f"cna inside {p['cna_cutoff']:.3f}, fitted {p['fitted']}")
    return (f"{spec['id']} size {spec['size']} tilt {spec['tilt'] is not None} relabel {spec['relabel']} free {spec['nonperiodic']} drift {spec['drift']} "
            f"steps {spec['nsteps']} rebuild {spec['rebuild']} read also at {spec['between']} rcap {spec['rcap']:.2f} seed {spec['seed']} "
            f"first: {text(spec['first'])}; " + (f"second: {text(spec['second'])}" if spec["second"] else "then off and the first again")
            + f"; reread {err['reread']} tags {err['tags']} owned once {not err['not_owned_once']} outside {err['outside']} coord {err['coord']} "
            f"integers {err['integers']} centro {err['centro']} short {err['short']} few {err['few']} refused {err['refused']} cna {err['cna']} "
            f"census {err['census']} over {err['over']} fresh {err['fresh']} edge {err['edge']} late {err['late']} builds {err['builds']} "
            f"worst centro error / bound {err['worst']:.3f}, most inside {err['most']}, most few {err['most_few']}, most over {err['most_over']}, "
            f"fewest centres with N inside {err['centres']}" + "".join("  " + f for f in err["failed"]))


# ---------------------------------------------------------------------------------------------------------- postforce
# The two post-force stages -- the indenters (csrc/indent.hip), the tether springs (csrc/spring.hip) and the life cycle they
# share (csrc/postforce.hip) -- on the three one-rank paths of the heat net ("hostlinked": indenters alone, the library
# refuses springs there) against tests/springref.host_spring, which adds indentref.post_force and springref.post_force to
# the ORACLE's forces: 0 - 4 indenters of every shape x side x dim the kernel tells apart on shuffled bits of HEAT_BITS (a
# bit-0 slot behind a slot with a bit), K from {0, 5, 20}, static or moving; 0 - 4 springs on shuffled bits of
# PF_SPRING_BITS or bit 0, groups that share atoms, every non-empty `use`, K from {0, 1, 10}, R0 zero, below or above the
# start distance, start image flags; REBO-MoS (its box has xy = -xprd / 2) and the alloy -- half of its cells sheared in all
# three tilts, a quarter with a free dimension (static: the states right behind the setup, the per[] == 0 branch of
# indent_minimum_image); first steps up to 2^32 + 7; optionally a second run behind step k (mdp_indent_run and
# mdp_spring_run of the stages that are on, in either order -- a second `run` sets up every fix, and a stage whose _run is
# left out would keep `applied` set across the compute that follows) over a pending or a completed final half, and a new
# mask at a read that leaves one spring's bit on no atom.
# Centres, radii, plane coordinates, tether points and velocities are FITTED to the start positions (_pf_system), not drawn:
# an indenter sits on a drawn site and reaches PF_PEN into its second atom, a moving one travels PF_TRAVEL relative to the
# crystal, a fraction of the spheres and cylinders is moved by a whole box vector (D then takes the wrap); a spring starts
# min(0.6, 0.6 atoms / K) A off its rest length.  One spring's group starts with a drift; where that group is the whole
# cell and every atom is integrated the crystal travels PF_DRIFT in the run (along z in a sheared cell, so that the remap
# carries the tilts into the image flags) and the indenters travel with it.  A plane's coordinate is taken raw by the
# kernel, and the device and the reference wrap at different steps: an atom of a plane's group next to a face would differ
# by a box vector in bookkeeping, not in physics, so a plane acts on the atoms that stay PF_FACE + skin away from every
# face whose remap changes the coordinate along `dim` (the faces along dim; in a sheared box those of the later dimensions
# too).  The r == 0 contact is a static sphere with side OUT centred on a held atom: dr = -R < 0 counts -K/3 dr^3 with no
# force (with side in, dr = R - 0 > 0 is no contact at all).
# At every read, the setup's (step 0) among them: x (minimum image) and v by tag, every state word of every indenter and
# spring (contacts, atoms, M, step and passes exact; centre and tether point to 1e-12 A), the atoms outside the integrate
# group bit for bit, no late check.
# Limits: see PF_LIMITS below.
PF_COMBOS = ((("sphere", "out", 0), ("sphere", "in", 0)) + tuple(("cylinder", sd, d) for sd in ("out", "in") for d in range(3))
             + tuple(("plane", sd, d) for sd in ("lo", "hi") for d in range(3)))
PF_SPRING_BITS = (128, 256, 512, 1024, 2048)
PF_USE = tuple((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or c)
PF_PEN = 0.25        # A: how far an indenter reaches into its second atom at the start
PF_GAP = 0.15        # A: its first and second atom are no further apart than this
PF_TRAVEL = 0.15     # A: what a moving indenter travels relative to the crystal in the run
PF_DRIFT = 1.6       # A: what a crystal that drifts as a whole travels in the run
PF_FACE = 1.5        # A: a plane's atoms stay skin + this away from the faces
PF_MILD = 2.0        # A/ps: the drift of a spring's group that is a part of the cell
# The limits (the reference's, not the device's).  *0: the state words at the setup read, where device and reference hold
# the same positions bit for bit; without: at the reads of the run.  Start: the bounds of tests/test_gpu_indent_mdp.py and
# tests/test_gpu_spring_mdp.py (1e-9 A, 2e-8 A/ps, 1e-12 of the terms, xcm 7.9e-12 A, E 9.5e-10 eV, ftotal 2.0e-10 eV/A).
# tests/test_net_draws.py::test_postforce_limits_are_the_references runs, over the suite's cases, (i) the reference with
# every stage's atoms summed in a random order and (ii) the reference with +-1e-9 eV/A on every force component; a bound
# stays if (i) is 100 times and (ii) 4 times inside it, else it is the larger of 100 x (i) and 4 x (ii), rounded up.
PF_START = dict(dx=1e-9, dv=2e-8, ie=1e-12, iforce=1e-12, sxcm=7.9e-12, se=9.5e-10, sf=2.0e-10,
                ie0=1e-12, iforce0=1e-12, sxcm0=7.9e-12, se0=9.5e-10, sf0=2.0e-10)
# Seed 44, 16 cases: the worst of (i) is dx 7.11e-15 A, dv 2.12e-13 A/ps, energy 8.82e-16 and force 5.58e-16 of an
# indenter's terms, xcm 4.26e-14 A, E 1.49e-13 eV, ftotal 2.49e-13 eV/A (at the setup read 4.21e-16, 1.23e-16, 7.82e-14 A,
# 1.49e-13 eV, 2.49e-13 eV/A): every bound holds it 100 times over.  The worst of (ii) is dx 3.13e-10 A, dv 1.14e-8 A/ps,
# indenter energy 1.36e-9 and force 3.55e-9 of their terms, xcm 3.10e-11 A, E 5.82e-11 eV, ftotal 1.02e-10 eV/A, and nothing
# at the setup read, which comes before any kick.  All but E are more than a quarter of the bounds -- K dr^2 and -K/3 dr^3
# follow an atom 0.25 A deep in a wall of K = 20 eV/A^3 at 10 eV/A^2 per A of its position, against terms of 0.1 eV --, so
# at the reads of the run six limits are four times that worst; E and the five of the setup read keep the project's bounds.
# Whoever changes the seed, the case count, the draw or the oracle's rounding measures both experiments again (the test
# prints their worst per quantity) and sets these numbers and DESIGN.md section 5 from what it prints.
# Measured on an MI355X (seed 44, 16 cases): 5.0e-14 A, 2.0e-12 A/ps, 1.9e-13 and 1.3e-13 of the indenter terms, xcm
# 3.6e-14 A, E 5.3e-14 eV, ftotal 1.1e-13 eV/A; at the setup read 1.1e-15, 8.7e-16, 6.9e-14 A, 9.0e-14 eV, 1.5e-13 eV/A;
# every exact word equal, no late check.  The limits are the reference's, not the device's.
PF_LIMITS = dict(PF_START, dx=1.3e-9, dv=4.6e-8, ie=5.5e-9, iforce=1.5e-8, sxcm=1.3e-10, sf=4.1e-10)


def draw_postforce(rng):
    style = rng.choice(["rebomos", "aeam"])
    free = None
    if style == "rebomos":
        size = rng.choice([(1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 2, 1)])
        spec = dict(size=size, n=_rebo_n(size), frac=None, tilt=None, skin=2.0)
    else:
        size, frac = rng.choice([4, 5, 6, 7]), rng.choice([0.0, 0.03])
        spec = dict(size=size, n=4 * size ** 3, frac=frac, tilt=None, skin=1.0)
        u, tilt, dim = rng.random(), [rng.uniform(-0.06, 0.06) * 4.045 * size for _ in range(3)], rng.randrange(3)
        if u < 0.25:     # one free dimension: a static case
            free = dim
        elif u < 0.75:   # sheared, all three tilts
            spec["tilt"] = tilt
    temp = rng.choice([300.0, 900.0])
    path = "resident" if free is not None else rng.choice(HEAT_PATHS)
    first = rng.choice(HEAT_FIRST)
    nsteps, dt = rng.choice([40, 60, 100]), rng.choice([0.0005, 0.001, 0.002])
    group = rng.choice(["all", "slab"])
    nind, nspr = rng.randrange(5), rng.randrange(5)
    if path == "hostlinked":
        nspr = 0
    if free is not None or nind + nspr == 0:
        nind = max(nind, rng.randint(1, 4))
    # the springs
    sbits = list(PF_SPRING_BITS)
    rng.shuffle(sbits)
    springs = []
    for k in range(nspr):
        q = dict(use=rng.choice(PF_USE), k=rng.choice([0.0, 1.0, 10.0]), r0=rng.choice(["zero", "below", "above"]), moving=rng.random() < 0.5,
                 kind=rng.choice(["everything", "modulus", "slab", "tiny"]), axis=rng.randrange(3), width=rng.choice([0.15, 0.25]),
                 count=rng.choice([2, 3]), pick=rng.randrange(10**6), u=[rng.uniform(-1.0, 1.0) for _ in range(3)], bit=sbits[k])
        springs.append(q)
    drifting, sign, whole, zero_bit = rng.randrange(max(nspr, 1)), rng.choice([-1, 1]), rng.random() < 0.5, rng.random() < 0.5
    if nspr and whole:   # the drifting spring holds the whole cell and every atom is integrated: the crystal travels
        springs[drifting]["kind"], group = "everything", "all"
    for q in springs:
        if q["kind"] == "everything" and zero_bit:
            q["bit"] = 0
    img = rng.random() < 0.5
    # the indenters
    bits = list(HEAT_BITS)
    rng.shuffle(bits)
    inds = []
    for k in range(nind):
        shape, side, dim = rng.choice(PF_COMBOS)
        if free is not None and k == 0:     # the one that decides per[]: it takes a minimum image along the free dimension
            shape, side, dim = rng.choice([c for c in PF_COMBOS if c[0] == "sphere" or (c[0] == "cylinder" and c[2] != free)])
        inds.append(dict(shape=shape, side=side, dim=dim, k=rng.choice([0.0, 5.0, 5.0, 20.0, 20.0]), moving=rng.random() < 0.5,
                         site=rng.choice(["atom", "interstitial"]),
                         shift=(rng.randrange(3), rng.choice([-1, 1])) if rng.random() < (0.8 if spec["tilt"] else 0.4) else None,
                         members=rng.choice(["all", "twothirds", "evens"]), r_plane=rng.choice([0.0, 3.0]), pick=rng.randrange(10**6),
                         w=[rng.uniform(-1.0, 1.0) for _ in range(3)], bit=bits[k]))
    # bit 0 behind a slot with a bit; never a plane: its atoms are chosen (see above), and bit 0 is every atom
    behind, rzero = rng.choice([k for k in range(1, nind) if inds[k]["shape"] != "plane"] or [None]), rng.random() < 0.3
    if behind is not None and rng.random() < 0.3:
        inds[behind]["bit"] = 0
    if free is not None and inds[0]["k"] == 0.0:
        inds[0]["k"] = 5.0
    if rzero and nind and group == "slab" and free is None:    # r == 0: a static sphere, side out, on a held atom
        inds[0].update(shape="sphere", side="out", dim=0, k=5.0, moving=False, site="held", shift=None, members="all")
    # thermo reads at random steps, the last step among them; True: the read finds the step's final half deferred and
    # completes it (passes included), False: the final half ran on its own before the read
    reads = [(st, rng.random() < 0.5) for st in sorted(rng.sample(range(1, nsteps), rng.randint(1, 4))) + [nsteps]]
    cut = None
    k, pending, order = rng.randrange(2, nsteps - 1), rng.random() < 0.5, rng.choice(["indent", "spring"])
    # a second run behind step k: the centres start again at c, so not where the crystal travels and would leave them behind
    if rng.random() < 0.4 and not (nspr and whole and nind):
        cut = (k, not pending or path == "hostlinked" or k in dict(reads), order)
    newmask = None
    at, which = rng.randrange(len(reads)), rng.randrange(max(nspr, 1))
    if nspr and rng.random() < 0.25 and at < len(reads) - 1 and springs[which]["bit"]:
        newmask = (reads[at][0], which)      # behind that read spring `which` has its bit on no atom
    if free is not None:
        nsteps, reads, cut, newmask = 0, [], None, None
    spec.update(style=style, temp=temp, path=path, free=free, first=first, nsteps=nsteps, dt=dt, group=group, inds=inds, springs=springs,
                drifting=drifting, sign=sign, img=img, reads=reads, cut=cut, newmask=newmask, renb=rng.choice([3, 5, 8]),
                seed=rng.randrange(1, 10**6), env={},
                id=f"{style}-{path}-n{spec['n']}-{group}" + ("-tilt" if spec["tilt"] else "") + (f"-free{free}" if free is not None else "")
                   + "-" + ".".join(q["shape"][0] + q["side"][0] + "xyz"[q["dim"]] for q in inds) + f"-spr{nspr}-first{first}-dt{dt}"
                   + (f"-cut{cut[0]}{'' if cut[1] else 'p'}" if cut else "") + ("-newmask" if newmask else ""))
    return spec


def _pf_unit(u, keep=(1, 1, 1)):
    u = np.where(np.array(keep, dtype=bool), np.array(u, dtype=float), 0.0)
    n = float(np.sqrt((u * u).sum()))
    if n < 1e-3:     # (nothing left of the drawn direction in the dimensions kept: the first of them)
        u = np.zeros(3)
        u[int(np.flatnonzero(keep)[0])] = 1.0
        return u
    return u / n


def pf_plane_faces(box, dim):
    """the dimensions whose faces a plane's atoms keep away from: a remap across them changes the coordinate along dim"""
    h = box.h
    return [e for e in range(dim, 3) if e == dim or h[dim, e] != 0.0]


def pf_face_distance(box, x, faces):
    """per atom the distance to the nearest face of the dimensions `faces` (negative outside the box)"""
    lam = box.x2lamda(x)
    hinv = box.hinv
    d = np.full(len(lam), np.inf)
    for e in faces:
        width = 1.0 / float(np.sqrt((hinv[e] ** 2).sum()))
        d = np.minimum(d, np.minimum(lam[:, e], 1.0 - lam[:, e]) * width)
    return d


def _pf_fit_round(s, x0, member, q, per, held, toward, decides, off):
    """centre and radius of a sphere or cylinder: from the drawn site on -- an atom's, or half way from an atom to one of its
    three nearest -- the first site at which the second atom (side in: the second farthest) is within PF_GAP of the first, or
    else the best one within twice that; the radius reaches PF_PEN into the second.  toward = (free dimension, unit vector out
    of a free face): the sites of a static case, next to that face and 1 A outside it; decides: ... at which other atoms
    would be in contact if the wrap were taken along the free dimension too; off: the box vector the centre is moved by (the
    fit is that of the moved centre: Domain::minimum_image takes one wrap per dimension, and an atom more than 1.5 boxes away
    keeps an image that is not its nearest).  In a box with tilts the image an atom takes changes r by a jump where the atom
    crosses half a box in y or z: a site is left out if a relative motion of 0.8 A along y or z takes an atom of the group that
    much deeper into contact and a jump more"""
    import indentref
    cyl, dim, out = q["shape"] == "cylinder", q["dim"], q["side"] == "out"

    def radial(c, periodic):
        d = x0 - c
        if cyl:
            d[:, dim] = 0.0
        d = indentref.minimum_image(s.box, d, periodic)
        return np.sqrt((d * d).sum(axis=1))

    perm = np.random.default_rng(q["pick"]).permutation(s.n)
    if toward is not None:
        lam = s.box.x2lamda(x0)[:, toward[0]]
        near = 3.0 / float(s.box.prd[toward[0]])
        perm = np.array([i for i in perm if (lam[i] < near if toward[1][toward[0]] < 0.0 else lam[i] > 1.0 - near)])
    sites = ["held"] if q["site"] == "held" else [q["site"]] + [k for k in ("interstitial", "atom") if k != q["site"]]
    best = None
    for site, nth, i in [(site, nth, i) for site in sites for nth in ((0, 1, 2) if site == "interstitial" else (0,)) for i in perm[:400]]:
        if site == "held" and not held[i]:
            continue
        c = x0[i].copy()
        if site == "interstitial":
            dn = indentref.minimum_image(s.box, x0 - x0[i], per)
            rn = np.sqrt((dn * dn).sum(axis=1))
            ok = rn > 0.1 if toward is None else (rn > 0.1) & (np.abs(dn[:, toward[0]]) < 0.1)      # (static: of the same layer)
            if ok.sum() <= nth:
                continue
            c += 0.5 * dn[int(np.argsort(np.where(ok, rn, np.inf), kind="stable")[nth])]
        if toward is not None:
            c += toward[1]
        c += off
        r = radial(c, per)
        m = member.copy()
        if site == "held":
            m[i] = False
        rs = np.sort(r[m])
        gap = float(rs[1] - rs[0] if out else rs[-1] - rs[-2])
        R = float(rs[1] + PF_PEN if out else rs[-2] - PF_PEN)
        if R <= 0.0 or (out and rs[0] < 0.5):      # (side out: not on an atom of the group, or on a column of them)
            continue
        if gap > PF_GAP:
            if not decides and gap <= 2.0 * PF_GAP and (best is None or gap < best[0]):
                best = (gap, c, R)
            continue
        if decides and np.array_equal((radial(c, (True, True, True)) < R) & m, (r < R) & m):
            continue
        if s.box.tilt.any():
            deep = np.maximum(R - r if out else r - R, 0.0)[m]
            if any(((R - ra if out else ra - R)[m] > deep + 0.85).any()
                   for ra in (radial(c + sg * 0.8 * np.eye(3)[e], per) for e in (1, 2) for sg in (-1.0, 1.0))):
                continue
        return c, R
    if best is not None:
        return best[1], best[2]
    raise AssertionError(f"no site fits the indenter {q}")


def _pf_system(spec):
    """no GPU, no oracle: the case as both sides take it -- dict(s, v0, x_in, by_tag, by_tag2: the new mask or None, g, ibit:
    the integrate bit, img0 [n][3], inds / springs: the reference's dicts (group: a boolean array, None with bit 0), dinds /
    dsprings: the device's, springs2: the reference's behind the new mask, per: the periodicity, safe: the steps between
    forced list builds by the _lgv_system rule, rigid: the velocity of a crystal that travels as a whole)"""
    import groupref
    import springref
    af = _res()["af"]
    free, skin, dt = spec["free"], spec["skin"], spec["dt"]
    if spec["style"] == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), spec["size"])
    else:
        s = S.fcc_cell(4.045, spec["size"], frac_type2=spec["frac"], seed=spec["seed"]); s.mass[1:3] = af.mass[:2]
        if spec["tilt"] is not None:     # (the sites a quarter of the lattice constant off the faces: see _heat_system)
            nb = S.Box(s.box.lo.copy(), s.box.prd.copy(), np.array(spec["tilt"]))
            s = S.System(nb, nb.lamda2x(s.box.x2lamda(s.x) + 0.25 / spec["size"]), s.type, s.tag, s.mass)
    assert s.n == spec["n"] and np.array_equal(s.tag, np.arange(1, s.n + 1))
    n, box = s.n, s.box
    x0 = S.wrap(box, s.x)
    lam = box.x2lamda(x0)
    mass = s.mass[s.type]
    per = tuple(d != free for d in range(3))
    g = np.ones(n, dtype=bool) if spec["group"] == "all" else groupref.masks(s)[1]
    T = max(spec["nsteps"], 1) * dt
    img0 = np.random.default_rng(spec["seed"] + 4).integers(-2, 3, (n, 3)) if spec["img"] else np.zeros((n, 3), dtype=np.int64)
    v0 = S.gaussian_velocities(s, spec["temp"], seed=spec["seed"] + 1)
    # the springs' groups, the drift
    sgroups = []
    for k, q in enumerate(spec["springs"]):
        a = lam[:, q["axis"]]
        if q["kind"] == "everything":
            l = np.ones(n, dtype=bool)
        elif q["kind"] == "modulus":
            l = s.tag % 3 == 0
        elif q["kind"] == "slab":
            rank = np.empty(n)         # contiguous along the axis: whole planes of the crystal, a plane cut at the ends
            rank[np.argsort(a, kind="stable")] = np.arange(n) / n
            l = (rank >= 0.2 * k) & (rank < 0.2 * k + q["width"])
        else:                          # 2 or 3 integrated atoms, no two of them within 6 A of each other
            r = np.random.default_rng(q["pick"])
            l = np.zeros(n, dtype=bool)
            for i in r.permutation(np.flatnonzero(g)):
                d = x0[l] - x0[i]
                d = d - np.round(box.x2lamda(d + box.lo)) @ box.h.T
                if not l.any() or float(np.sqrt((d ** 2).sum(axis=1)).min()) > 6.0:
                    l[i] = True
                if l.sum() == q["count"]:
                    break
        assert l.sum() >= 2, (spec["id"], k, q["kind"], int(l.sum()))
        sgroups.append(l)
    rigid = np.zeros(3)
    if spec["springs"] and spec["nsteps"]:
        q = spec["springs"][spec["drifting"]]
        axis = 2 if spec["tilt"] is not None else q["axis"]
        if q["kind"] == "everything" and spec["group"] == "all":
            rigid[axis] = spec["sign"] * PF_DRIFT / T
            v0 += rigid
        else:
            v0[sgroups[spec["drifting"]] & g, axis] += spec["sign"] * PF_MILD
    # the indenters: groups, centres, radii, velocities
    toward = None
    if free is not None:
        e = np.zeros(3)
        e[free] = -1.0 if spec["sign"] < 0 else 1.0
        toward = (free, e)
    inds, dinds = [], []
    for k, q in enumerate(spec["inds"]):
        dim, vel = q["dim"], rigid.copy()
        w = _pf_unit(q["w"])
        if q["shape"] == "plane":
            faces = pf_plane_faces(box, dim)
            room = skin + PF_FACE + 0.8 + (PF_DRIFT if rigid.any() else 0.0)      # (0.8 A: what thermal motion may take)
            member = pf_face_distance(box, x0, faces) >= room
            lo = q["side"] == "lo"
            while member.sum() >= 4:       # atoms that stand out of the first layer by more than PF_GAP leave the group
                idx = np.flatnonzero(member)
                xs = x0[idx, dim]
                o = np.argsort(xs if lo else -xs, kind="stable")
                if abs(xs[o[1]] - xs[o[0]]) <= PF_GAP:
                    break
                member[idx[o[0]]] = False
            assert member.sum() >= 4, (spec["id"], k, "no atoms for the plane", int(member.sum()))
            c = np.array([0.3, -0.7, 1.1])   # (the kernel reads the component along dim alone)
            c[dim] = xs[o[1]] + PF_PEN if lo else xs[o[1]] - PF_PEN
            if q["moving"]:
                vel[dim] += (1.0 if w[dim] >= 0.0 else -1.0) * PF_TRAVEL / T
            r = q["r_plane"]
        else:
            member = {"all": np.ones(n, dtype=bool), "twothirds": s.tag % 3 != 1, "evens": s.tag % 2 == 0}["all" if q["bit"] == 0 else q["members"]]
            off = q["shift"][1] * box.h[:, q["shift"][0]] if q["shift"] is not None and q["shift"][0] != free else np.zeros(3)
            c, r = _pf_fit_round(s, x0, member, q, per, ~g, toward, toward is not None and k == 0, off)
            if q["moving"]:
                vel += w * PF_TRAVEL / T
            if q["shape"] == "cylinder":
                vel[dim] = 0.0
        d = dict(shape=q["shape"], side=q["side"], dim=dim, k=q["k"], r=float(r), c=tuple(float(a) for a in c), vel=tuple(float(a) for a in vel),
                 bit=q["bit"])
        dinds.append(d)
        inds.append(dict(d, group=None if q["bit"] == 0 else member))
    # the springs: tether points, rest lengths, velocities
    xu0 = springref.unwrap(box, x0, img0)
    springs, dsprings = [], []
    for k, (q, l) in enumerate(zip(spec["springs"], sgroups)):
        m = mass[l]
        xcm = (m[:, None] * xu0[l]).sum(axis=0) / m.sum()
        u = _pf_unit(q["u"], q["use"])
        off = min(0.6, 0.6 * int(l.sum()) / q["k"]) if q["k"] else 0.3
        dist, r0 = {"zero": (off, 0.0), "below": (2.0 * off, off), "above": (0.5, 0.5 + off)}[q["r0"]]
        c = tuple(float(xcm[e] + dist * u[e]) if q["use"][e] else None for e in range(3))
        vel = np.where(np.array(q["use"], dtype=bool), rigid + (u * 0.3 / T if q["moving"] else 0.0), 0.0)
        d = dict(k=q["k"], r0=r0, c=c, vel=tuple(float(a) for a in vel), bit=q["bit"])
        dsprings.append(d)
        springs.append(dict(d, group=None if q["bit"] == 0 else l))
    by_tag = np.zeros(n + 1, dtype=np.int32)
    mk = groupref.ALL_BIT | np.where(g, groupref.INTEGRATE_BIT, 0)
    for q in inds + springs:
        if q["bit"]:
            mk = mk | np.where(q["group"], q["bit"], 0)
    by_tag[s.tag] = mk
    by_tag2 = springs2 = None
    if spec["newmask"] is not None:
        e = spec["newmask"][1]
        by_tag2 = by_tag & ~np.int32(springs[e]["bit"])
        springs2 = [dict(q, group=np.zeros(n, dtype=bool)) if j == e else q for j, q in enumerate(springs)]
    vcap = float(np.sqrt((v0 ** 2).sum(axis=1)).max()) + 5.0 * np.sqrt(S.BOLTZ * 1.5 * spec["temp"] / (float(s.mass[1:3].min()) * S.MVV2E))
    safe = max(1, int(0.3 * skin / (vcap * dt)))
    return dict(s=s, v0=v0, x_in=x0, by_tag=by_tag, by_tag2=by_tag2, g=g, ibit=0 if spec["group"] == "all" else groupref.INTEGRATE_BIT, img0=img0,
                inds=inds, dinds=dinds, springs=springs, dsprings=dsprings, springs2=springs2, per=per, safe=safe, rigid=rigid)


def postforce_reference(spec, P=None, permuted=False, dforce=0.0, periodic=None):
    """no GPU: springref.host_spring of the case around the oracle; ({read step, 0 among them: (x, spring states, v, xu,
    indenter states)}, what the run showed: per indenter fmax, deepest (over the atoms with r > 0), the most contacts of a
    read, the dimensions in which an atom in contact took the wrap, the least distance of a plane's atoms from their
    faces; per spring fmax; whether an atom of a spring's group changed its z image flag in mid-run).
    permuted: every stage's atoms summed in a random order (experiment (i)); dforce: experiment (ii); periodic: instead of
    the case's own"""
    import indentref
    import mdref
    import springref
    R = _res()
    P = P or _pf_system(spec)
    s, skin, nsteps = P["s"], spec["skin"], spec["nsteps"]
    per = P["per"] if periodic is None else periodic
    make = ((lambda sy: mdref.RebomosCPU(R["orc"], R["P"], sy, skin=skin)) if spec["style"] == "rebomos" else
            (lambda sy: mdref.AeamCPU(R["orc"], R["T"], sy, skin=skin)))
    orders = ind_orders = None
    if permuted:
        r = np.random.default_rng(spec["seed"] + 2)
        orders, ind_orders = [r.permutation(s.n) for _ in P["springs"]], [r.permutation(s.n) for _ in P["inds"]]
    ni = len(P["inds"])
    seen = dict(fmax=[0.0] * ni, deepest=[0.0] * ni, contacts=[0] * ni, wraps=[set() for _ in range(ni)], face=[np.inf] * ni, zflag=False,
                rzero=False)
    ingroup = np.zeros(s.n, dtype=bool)
    for q in P["springs"]:
        ingroup |= np.ones(s.n, dtype=bool) if q["group"] is None else q["group"]
    reads = {0} | set(dict(spec["reads"]))

    def on_force(step, x, img, st, ist):
        for k, (q, w) in enumerate(zip(P["inds"], ist)):
            taken = {}
            dr, _, r = indentref.depth(q, w["centre"], s.box, x, per, taken)
            on = dr < 0.0 if q["group"] is None else (dr < 0.0) & q["group"]
            seen["fmax"][k] = max(seen["fmax"][k], w["fmax"])
            if (on & (r > 0.0)).any():
                seen["deepest"][k] = max(seen["deepest"][k], float(-dr[on & (r > 0.0)].min()))
            seen["rzero"] = seen["rzero"] or bool((on & (r == 0.0)).any() and q["k"] > 0.0)
            if step in reads:
                seen["contacts"][k] = max(seen["contacts"][k], w["contacts"])
            seen["wraps"][k] |= {e for e, sg in taken.items() if (sg[on] != 0.0).any()}
            if q["shape"] == "plane":
                seen["face"][k] = min(seen["face"][k], float(pf_face_distance(s.box, x[q["group"]], pf_plane_faces(s.box, q["dim"])).min()))
        if 0 < step < nsteps and (img[:, 2] != P["img0"][:, 2])[ingroup & P["g"]].any():
            seen["zflag"] = True

    regroup = None if spec["newmask"] is None else {spec["newmask"][0]: (P["springs2"], P["inds"])}
    out, w = springref.host_spring(make, s, P["v0"], P["img0"], nsteps, reads, min(LGV_REBUILD[spec["style"]], P["safe"]), P["g"], P["springs"],
                                   dt=spec["dt"], first=spec["first"], orders=orders, cut=None if spec["cut"] is None else spec["cut"][0],
                                   inds=P["inds"], ind_orders=ind_orders, dforce=dforce, regroup=regroup, skin=skin if nsteps else None,
                                   on_force=on_force, periodic=per, keep_held=True)
    seen.update(sfmax=w["fmax"], flagged=w["flagged"])
    return out, seen


def postforce_worst(spec, P, ref, dev, held=False):
    """the worst deviations of {step: (x, spring states, v, xu, indenter states)} `dev` from `ref` over the reads: dx, dv;
    an indenter's energy and force as fractions of the sums of the magnitudes of their terms, a spring's xcm, E and ftotal
    absolute (at step 0 under the names that end in 0); `exact`: the words that must agree exactly and do not (contacts,
    atoms, M; of a device state also step and passes, and centre and tether point beyond 1e-12 A); with held: the reads at
    which an atom outside the integrate group is not where, and as fast as, it was put"""
    import refloops
    s, g = P["s"], P["g"]
    w = dict.fromkeys(PF_START, 0.0)
    exact = nheld = 0
    k_cut = spec["cut"][0] if spec["cut"] else None
    for step in ref:
        xh, sh, vh, _, ih = ref[step]
        xd, sd, vd, _, idv = dev[step]
        z = "0" if step == 0 else ""
        d = xd - xh
        d = d - np.round(s.box.x2lamda(d + s.box.lo)) @ s.box.h.T
        w["dx"] = refloops.worse(w["dx"], float(np.abs(d).max()))
        w["dv"] = refloops.worse(w["dv"], float(np.abs(vd - vh).max()))
        passes = step + 1 + (1 if k_cut is not None and step > k_cut else 0)
        exact += int(len(idv) != len(ih)) + int(len(sd) != len(sh))
        for a, b in zip(idv, ih):
            te, tf = b["terms"]
            w["ie" + z] = refloops.worse(w["ie" + z], abs(a["energy"] - b["energy"]) / te if te else abs(a["energy"]))
            for c in range(3):
                w["iforce" + z] = refloops.worse(w["iforce" + z], abs(a["force"][c] - b["force"][c]) / tf[c] if tf[c] else abs(a["force"][c]))
            exact += int(a["contacts"] != b["contacts"])
            if "passes" in a:
                exact += int(a["step"] != spec["first"] + step) + int(a["passes"] != passes) + int(not np.abs(a["centre"] - b["centre"]).max() <= 1e-12)
        for a, b in zip(sd, sh):
            w["sxcm" + z] = refloops.worse(w["sxcm" + z], float(np.abs(a["xcm"] - b["xcm"]).max()))
            w["se" + z] = refloops.worse(w["se" + z], abs(a["energy"] - b["energy"]))
            w["sf" + z] = refloops.worse(w["sf" + z], float(np.abs(np.asarray(a["ftotal"]) - b["ftotal"]).max()))
            exact += int(a["atoms"] != b["atoms"]) + int(a["mass"] != b["mass"])
            if "passes" in a:
                exact += int(a["step"] != spec["first"] + step) + int(a["passes"] != passes) + int(not np.abs(a["tether"] - b["tether"]).max() <= 1e-12)
        if held:
            nheld += int(not (np.array_equal(xd[~g], P["x_in"][~g]) and np.array_equal(vd[~g], P["v0"][~g])))
    w.update(exact=exact)
    if held:
        w.update(held=nheld)
    return w


def _pf_resident(spec, P, rebuild_every):
    """one resident brick.  rebuild_every None: the device's own check; a number: the integrate calls without the check,
    reneighbourings forced every so many steps"""
    from lammps_plugins_amd.host import resident
    s, reads, cut, ni, ns = P["s"], dict(spec["reads"]), spec["cut"], len(P["dinds"]), len(P["dsprings"])
    ctx, st, cutghost, map_ = _lgv_context(spec["style"])

    def read(d):
        ists = [ctx.indent_state(k) for k in range(ni)]     # (the indenters' first: the read of either kind runs both passes)
        ssts = [ctx.spring_state(k) for k in range(ns)]
        got = ctx.md_download(d.nlocal, want=("x", "v"))
        x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
        x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
        return (x, ssts, v, None, ists)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, spec["skin"], map_, v0=P["v0"], dt=spec["dt"],
                                  nonperiodic=tuple(0 if p else 1 for p in P["per"]))
        d.set_group(P["by_tag"], P["ibit"])
        if ns:
            d.track_images(resident.image_pack(P["img0"]))
        d.compute(1, 0)
        if ni:
            d.indent(P["dinds"], first=spec["first"])
        if ns:
            d.spring(P["dsprings"], first=spec["first"])
        out = {0: read(d)}
        for step in range(1, spec["nsteps"] + 1):
            rb = "auto" if rebuild_every is None else step % rebuild_every == 0
            defer = reads.get(step, True)
            if cut is not None and step == cut[0] and step not in reads:
                defer = not cut[1]
            d.step(0, 0, rebuild=rb, defer_final=defer)
            if step in reads:
                out[step] = read(d)
                if spec["newmask"] is not None and step == spec["newmask"][0]:
                    ctx.md_set_mask(P["by_tag2"][d.tags_local].astype(np.int32))
            if cut is not None and step == cut[0]:       # the second run: every stage that is on, then its setup's compute
                for kind in (("indent", "spring") if cut[2] == "indent" else ("spring", "indent")):
                    if (ni if kind == "indent" else ns):
                        getattr(d, kind + "_run")(spec["first"] + step)
                d.compute(0, 0)
        return out, d.builds, d.dangerous
    finally:
        ctx.close()


def _pf_hostlinked(spec, P, rebuild_every):
    """_heat_hostlinked with the indenters: a shuffled host order, host reneighbourings that upload atoms, velocities and
    mask again"""
    import ctypes as C
    import oracle_bindings as ob
    from lammps_plugins_amd.host import capi
    R = _res()
    s, g = P["s"], P["g"]
    style, n, skin, ni = spec["style"], s.n, spec["skin"], len(P["dinds"])
    rcut = (R["P"].cut3rebo if style == "rebomos" else float(R["af"].cut_table(R["tabs"]).max())) + skin
    perm = np.random.default_rng(spec["seed"] + 3).permutation(n)
    type_p, tag_p, gp = s.type[perm].copy(), s.tag[perm].copy(), g[perm]
    mask_p = P["by_tag"][tag_p]
    c = capi.Context(0)

    def upload(x, v):
        xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), type_p, tag_p, s.mass), rcut)
        c.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=[0, 0, 1] if style == "rebomos" else None)
        c.set_skin(skin)
        c.hnve_upload_v(v)

    def compute():   # f == NULL: the forces' only reader is the device's integrator
        if style == "rebomos":
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
        else:
            eng, vir = C.c_double(0.0), np.zeros(6)
            c._ck(c.L.mdp_aeam_density_host(c.h, C.c_int(0), None, None, C.byref(eng), None))
            c._ck(c.L.mdp_aeam_force_host(c.h, C.c_int(0), C.c_int(0), None, None, C.byref(eng), capi._dp(vir), None, None))

    def read():
        ists = [c.indent_state(k) for k in range(ni)]
        got = c.hnve_download(n, want=("x", "v"))
        x, v = np.zeros((n, 3)), np.zeros((n, 3))
        x[tag_p - 1], v[tag_p - 1] = got["x"], got["v"]
        return (x, [], v, None, ists)
    try:
        if style == "rebomos":
            c.rebomos_set_params(ob.product_rebomos_params(R["P"]))
        else:
            c.aeam_set_tables(R["tabs"]); c.aeam_device_lists(True)
        c.set_box_host(s.box)
        c.hnve_setup(spec["dt"], S.FTM2V, s.mass)
        c.integrate_group(P["ibit"])
        upload(P["x_in"][perm], P["v0"][perm])
        c.hnve_set_mask(mask_p)
        compute()
        c.indent_setup(P["dinds"])
        c.indent_run(spec["first"])
        reads, late_any, rebuilds = dict(spec["reads"]), 0, 0
        out = {0: read()}
        for step in range(1, spec["nsteps"] + 1):
            moved, late = c.hnve_initial()
            late_any += int(late)
            if moved or step % rebuild_every == 0:
                got = c.hnve_download(n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]     # (a host that wraps rewrites only atoms that left the box: the held ones did not)
                upload(xw, got["v"])
                c.hnve_set_mask(mask_p)
                rebuilds += 1
            compute()
            c.hnve_final()
            if step in reads:
                out[step] = read()
            if spec["cut"] is not None and step == spec["cut"][0]:
                c.indent_run(spec["first"] + step)
                compute()
    finally:
        c.close()
    return out, rebuilds, late_any


def run_postforce(spec):
    P = _pf_system(spec)
    forced, ref_every = min(spec["renb"], P["safe"]), min(LGV_REBUILD[spec["style"]], P["safe"])
    ref, seen = postforce_reference(spec, P)
    if spec["path"] == "hostlinked":
        dev, builds, late = _pf_hostlinked(spec, P, ref_every)
    else:
        dev, builds, late = _pf_resident(spec, P, None if spec["path"] == "resident" else forced)
    err = postforce_worst(spec, P, ref, dev, held=True)
    last = dev[spec["nsteps"]]
    err.update(late=late, builds=builds, contacts=[q["contacts"] for q in last[4]], atoms=[q["atoms"] for q in last[1]],
               deepest=max(seen["deepest"], default=0.0), sfmax=max(seen["sfmax"], default=0.0))
    return err, dict(PF_LIMITS, exact=1, held=1, late=1)


def line_postforce(spec, err):
    return (f"{spec['id']} steps {spec['nsteps']} T {spec['temp']:.0f} K {[q['k'] for q in spec['inds']]} bits {[q['bit'] for q in spec['inds']]} "
            f"springs {[(q['kind'], q['bit'], q['k'], q['r0']) for q in spec['springs']]} img {int(spec['img'])} reads {[(a, int(b)) for a, b in spec['reads']]} "
            f"seed {spec['seed']} " + " ".join(f"{k} {err[k]:.1e}" for k in PF_START) +
            f" contacts {err['contacts']} atoms {err['atoms']} deepest {err['deepest']:.2f} spring fmax {err['sfmax']:.2f} exact {err['exact']} "
            f"held {err['held']} late {err['late']} builds {err['builds']}")


# ---------------------------------------------------------------------------------------------------------------- nvt
# The Nose-Hoover chain thermostat (tests/test_gpu_nvt_net.py): chains of 1-8, 1-3 loops, drag, flat or ramped targets,
# both styles, the resident path and (REBO-MoS) the host-linked one, atom counts whose last 256-atom block varies.
NVT_SUITE = (25, 10)     # (seed, cases); tests/test_net_draws.py asserts the corners


def draw_nvt(rng):
    style = rng.choice(["rebomos", "aeam"])
    tchain, tloop, drag = rng.randint(1, 8), rng.randint(1, 3), rng.choice([0.0, 0.2, 0.5])
    t0 = rng.choice([300.0, 600.0])
    t1 = rng.choice([t0, 900.0])
    if style == "rebomos":
        size = rng.choice([(1, 1, 1), (2, 1, 1), (3, 1, 1)])
        n = REBO_CELL_N * size[0] * size[1] * size[2]
        path = rng.choice(["resident", "hostlinked"])
    else:
        size = rng.choice([4, 5, 6, 7])
        n = 4 * size ** 3
        path = "resident"
    return dict(style=style, path=path, tchain=tchain, tloop=tloop, drag=drag, t0=t0, t1=t1, size=size, n=n,
                seed=rng.randrange(1, 10**6))


def nvt_cases(seed, ncase):
    rng = random.Random(seed)
    return [draw_nvt(rng) for _ in range(ncase)]


NETS = {name: (globals()["draw_" + name], globals()["run_" + name], globals()["line_" + name])
        for name in ("force", "hostmode_walk", "aeam_types", "prune", "dd", "hnve", "minilmp", "trajectory", "block", "fire", "langevin", "heat", "measure", "peratom",
                     "structure", "postforce")}


def main(net, argv):
    """the command line of profiles/<net>_fuzz.py: <cases> <seed> [dd: style]; one line per case, exit status 1 if any
    case failed"""
    import sys
    import time
    ncase, seed = int(argv[0]), int(argv[1])
    draw, run, line = NETS[net]
    rng = random.Random(seed)
    only = argv[2] if net == "dd" and len(argv) > 2 else None
    bad = 0; t0 = time.time()
    for k in range(ncase):
        spec = draw_dd(rng, only) if net == "dd" else draw(rng)
        try:
            with knobs(spec["env"]):
                err, lim = run(spec)
            ok, text = passed(err, lim), line(spec, err)
        except Exception as e:  # noqa: BLE001
            ok, text = False, f"{spec['id']} exception {type(e).__name__} {str(e)[-300:]}"
        bad += 0 if ok else 1
        print(f"{'ok ' if ok else 'BAD'} case {k} {text}", flush=True)
    print(f"{ncase} cases, {bad} bad, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)
