"""The host reference of the constant-flux heat sources (tests/test_heatref.py, tests/test_gpu_heat_mdp.py, tests/nets.py): LAMMPS
FixHeat::end_of_step with a constant eflux and no region, restated, and the masked velocity-Verlet loops around it -- LAMMPS
`fix nve` on a group next to several `fix heat` on disjoint groups inside it.  A source is a dict
    dict(group=<boolean array>, eflux=<energy / time, either sign>, nevery=<steps between applications>)
Step n is heated after its final half if n % nevery == 0; step `first` of a run never is (Verlet::setup does not call
end_of_step).  A helper module, not a test module; no GPU."""
from __future__ import annotations

import numpy as np

from lammps_plugins_amd.host import system as S


class HeatError(RuntimeError):
    """LAMMPS' "Fix heat kinetic energy went negative" """


def kecm(v, m, group, ftm2v, mvv2e):
    """(ke - 0.5 vcm.vcm M) of FixHeat: the group's kinetic energy about its centre of mass, times ftm2v"""
    g = np.asarray(group, dtype=bool)
    mg, vg = m[g], v[g]
    M = float(mg.sum())
    ke = (0.5 * float(np.sum(mg[:, None] * vg * vg)) * mvv2e) * ftm2v
    vcm = (mg[:, None] * vg).sum(axis=0) / M
    return ke - 0.5 * float(vcm @ vcm) * M


def apply(v, m, group, eflux, nevery, dt, ftm2v, mvv2e, M=None, order=None):
    """one application on the atoms of `group`, in place; returns (scale, vcm, ke about the COM before it).  M: the mass
    LAMMPS takes once at init (summed here if None).  order: a permutation of the group's atoms to add them up in"""
    g = np.flatnonzero(np.asarray(group, dtype=bool))
    if order is not None:
        g = g[order]
    mg, vg = m[g], v[g]
    if M is None:
        M = float(mg.sum())
    heat = eflux * nevery * dt * ftm2v
    ke = (0.5 * float(np.sum(mg[:, None] * vg * vg)) * mvv2e) * ftm2v
    vcm = (mg[:, None] * vg).sum(axis=0) / M
    t = 0.5 * float(vcm @ vcm) * M
    den = ke - t
    escale = (ke + heat - t) / den
    if not den > 0.0 or not escale >= 0.0:
        raise HeatError("Fix heat kinetic energy went negative")
    scale = float(np.sqrt(escale))
    v[g] = scale * vg - (scale - 1.0) * vcm
    return scale, vcm, den


def end_of_step(n, v, m, sources, dt, ftm2v, mvv2e, masses=None, orders=None):
    """the sources that are due at step n, each on its own group; {k: (scale, vcm, ke about the COM, escale)}"""
    out = {}
    for k, s in enumerate(sources):
        if n % s["nevery"] == 0:
            r = apply(v, m, s["group"], s["eflux"], s["nevery"], dt, ftm2v, mvv2e, M=None if masses is None else masses[k],
                      order=None if orders is None else orders[k])
            out[k] = r + (r[0] * r[0],)
    return out


def run(x, v, m, force, sources, first, last, dt, ftm2v, mvv2e, group, on_step=None):
    """velocity Verlet on `group` with the sources, steps first + 1 .. last, in place; on_step(n, x, v, pe, applied)"""
    dtf = 0.5 * dt * ftm2v
    g = np.asarray(group, dtype=bool)
    mg = m[g][:, None]
    masses = [float(m[np.asarray(s["group"], dtype=bool)].sum()) for s in sources]
    f, pe = force(x)
    for n in range(first + 1, last + 1):
        v[g] += dtf * f[g] / mg
        x[g] += dt * v[g]
        f, pe = force(x)
        v[g] += dtf * f[g] / mg
        applied = end_of_step(n, v, m, sources, dt, ftm2v, mvv2e, masses)
        if on_step is not None:
            on_step(n, x, v, pe, applied)
    return x, v


def host_heat(make_engine, s, v0, nsteps, every, rebuild_every, group, sources, dt=0.001, orders=None, first=0, cut=None,
              skin=None, dforce=0.0, states=False):
    """groupref.host_group with the sources: velocity Verlet on `group` around the oracle, the lists built anew every
    rebuild_every steps; {step: (x by tag, [scale of source k's last application], v by tag)} for the steps in `every`, and
    the smallest escale of the run.  orders: per source a permutation its atoms are summed in (None: the order of s).
    The run's steps are numbered first + 1 .. first + nsteps as in run(): step `first` is never heated, step first + n is
    if (first + n) % nevery == 0.
    cut = (k, completed): the host starts a second run at step first + k of this one (mdp_heat_run(first + k)).  Step
    first + k belongs to the first run, whose end_of_step heats it; it is not heated again as the second run's first step.
    completed False: the host left that step's final half pending across the call -- the library completes it there
    WITHOUT the sources, so the applications of step first + k do not happen at all.
    skin: assert that no atom has moved more than half of it since the last build (refloops.host_lgv's rule).
    dforce: every force component of every step gets an error drawn uniformly from +-dforce (the experiment behind the
    nets' limits).
    states True: a fourth entry per read, [dict(scale, vcm, kecm, applied, due) of source k]: its last application (1, 0,
    0 before the first), its applications so far and whether it was due at the read step itself"""
    g = np.asarray(group, dtype=bool)
    m = s.mass[s.type]
    mg = m[g]
    masses = [float(m[np.asarray(q["group"], dtype=bool)].sum()) for q in sources]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    x_built = x.copy()
    noise = np.random.default_rng(20261) if dforce else None
    f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
    if dforce:
        f = f + noise.uniform(-dforce, dforce, f.shape)
    dtf = 0.5 * dt * S.FTM2V
    scales = [1.0] * len(sources)
    last = [dict(scale=1.0, vcm=np.zeros(3), kecm=0.0, applied=0, due=False) for _ in sources]
    out, lowest = {}, np.inf
    for step in range(1, nsteps + 1):
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
            x_built = x.copy()
        elif skin is not None:
            far = float(np.sqrt(((x - x_built) ** 2).sum(axis=1)).max())
            assert far <= 0.5 * skin, f"the reference's own list is stale at step {step}: an atom moved {far:.3f} A"
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
        if dforce:
            f = f + noise.uniform(-dforce, dforce, f.shape)
        v[g] += dtf * f[g] / mg[:, None]
        for q in last:
            q["due"] = False
        if cut is None or step != cut[0] or cut[1]:
            for k, r in end_of_step(first + step, v, m, sources, dt, S.FTM2V, S.MVV2E, masses, orders).items():
                scales[k] = r[0]
                lowest = min(lowest, r[3])
                last[k] = dict(scale=r[0], vcm=r[1].copy(), kecm=r[2], applied=last[k]["applied"] + 1, due=True)
        if step in every:
            out[step] = (x.copy(), list(scales), v.copy()) + (([dict(q) for q in last],) if states else ())
    return out, lowest
