"""The masked host loops of the group tests (tests/test_groupref.py, tests/test_gpu_group_mdp.py): velocity Verlet on a
group of atoms -- LAMMPS `fix ID GROUP nve / nvt / langevin` -- around tests/nhcref.py and tests/langevinref.py as they
are.  An atom outside the integrate group keeps x and v; the Nose-Hoover temperature, the Langevin force, its `zero` mean
and its tally run over their groups alone.  With an all-true mask every loop here is its all-atoms twin bit for bit
(tests/test_groupref.py).  A helper module, not a test module; no GPU."""
from __future__ import annotations

import numpy as np

from lammps_plugins_amd.host import system as S

ALL_BIT, INTEGRATE_BIT, LANGEVIN_BIT = 1, 2, 4


def masks(s):
    """(mask by TAG [n + 1], integrate group, Langevin group as boolean arrays in the order of s) of the group tests: the
    integrate group is everything but a z-slab of about a third of the cell and the atoms with tag % 5 == 0 -- in the
    device's Hilbert order whole 256-atom blocks of held atoms, waves with mixed lanes and a partial last block --, the
    Langevin group its atoms with an even tag.  Bit 1 is set on every atom, as in LAMMPS."""
    lam = s.box.x2lamda(S.wrap(s.box, s.x))
    g = ~(lam[:, 2] < 1.0 / 3.0) & (s.tag % 5 != 0)
    lg = g & (s.tag % 2 == 0)
    by_tag = np.zeros(int(s.tag.max()) + 1, dtype=np.int32)
    by_tag[s.tag] = ALL_BIT | np.where(g, INTEGRATE_BIT, 0) | np.where(lg, LANGEVIN_BIT, 0)
    return by_tag, g, lg


def check_masks(s, g, lg):
    """the conditions on the input every group test states before anything is launched"""
    assert 0.25 * s.n <= g.sum() <= 0.75 * s.n, (int(g.sum()), s.n)
    assert 0 < lg.sum() < g.sum(), (int(lg.sum()), int(g.sum()))
    assert not (lg & ~g).any()


# ---- the loops of nhcref / langevinref with a group (force(x) -> (f, pe); on_step(n, x, v, pe) after each step)
def run_nvt(x, v, m, force, nhc, first, last, ftm2v, group, on_step=None):
    """nhcref.run_nvt on the atoms of `group`; nhc.nf is the caller's (3 N_group - 3)"""
    dt = nhc.dt
    g = np.asarray(group, dtype=bool)
    mg = m[g]
    f, pe = force(x)
    nhc.setup(v[g], mg, first, last)
    dtf = 0.5 * dt * ftm2v
    for n in range(first + 1, last + 1):
        nhc.begin_step(n)
        v[g] *= nhc.half()
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        f, pe = force(x)
        v[g] += dtf * f[g] / mg[:, None]
        v[g] *= nhc.half(nhc.temperature(v[g], mg))
        if on_step is not None:
            on_step(n, x, v, pe)
    return x, v


def lgv_force(lgv, n, tag, type_, v, lgroup, phase=0):
    """the Langevin force of step n on every atom: langevinref's on the Langevin group (its `zero` mean then divides by
    the group's count, and lgv.fl -- what the tally sums -- holds the group's rows), nothing elsewhere"""
    l = np.asarray(lgroup, dtype=bool)
    fl = np.zeros_like(v)
    fl[l] = lgv.force(n, tag[l], type_[l], v[l], phase=phase)
    return fl


def run_langevin(x, v, mass_atom, tag, type_, force, lgv, first, last, ftm2v, group, lgroup, on_step=None):
    """langevinref.run_langevin with the integrator on `group` and the thermostat on `lgroup` (inside group)"""
    dt = lgv.dt
    dtf = 0.5 * dt * ftm2v
    g, l = np.asarray(group, dtype=bool), np.asarray(lgroup, dtype=bool)
    m = mass_atom[g][:, None]
    lgv.setup(first, last)
    f, pe = force(x)
    f = f + lgv_force(lgv, first, tag, type_, v, l, phase=1)
    lgv.tally_setup(v[l])
    for n in range(first + 1, last + 1):
        v[g] += dtf * f[g] / m
        x[g] += dt * v[g]
        f, pe = force(x)
        f = f + lgv_force(lgv, n, tag, type_, v, l)
        v[g] += dtf * f[g] / m
        lgv.tally_step(v[l])
        if on_step is not None:
            on_step(n, x, v, pe)
    return x, v


# ---- the same around the oracle engines of tests/mdref.py, with the lists built anew every rebuild_every steps
def host_group(make_engine, s, v0, nsteps, every, rebuild_every, group, nhc=None, lgv=None, lgroup=None, dt=0.001):
    """velocity Verlet on `group` around the oracle -- plain, with the chain `nhc` (a masked copy of _host_nvt of
    tests/test_gpu_nvt_mdp.py) or with the thermostat `lgv` on `lgroup` (tests/refloops.py host_lgv);
    {step: (x by tag, thermostat energy or tally or 0.0, T of the group or 0.0, v by tag)} for the steps in `every`"""
    g = np.asarray(group, dtype=bool)
    mg = s.mass[s.type][g]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
    if nhc is not None:
        nhc.setup(v[g], mg, 0, nsteps)
    if lgv is not None:
        lgv.setup(0, nsteps)
        f = f + lgv_force(lgv, 0, s.tag, s.type, v, lgroup, phase=1)
        lgv.tally_setup(v[lgroup])
    dtf = 0.5 * dt * S.FTM2V
    out = {}
    for step in range(1, nsteps + 1):
        if nhc is not None:
            nhc.begin_step(step)
            v[g] *= nhc.half()
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
        if lgv is not None:
            f = f + lgv_force(lgv, step, s.tag, s.type, v, lgroup)
        v[g] += dtf * f[g] / mg[:, None]
        if nhc is not None:
            v[g] *= nhc.half(nhc.temperature(v[g], mg))
        if lgv is not None:
            lgv.tally_step(v[lgroup])
        if step in every:
            e = nhc.energy() if nhc is not None else (lgv.scalar() if lgv is not None else 0.0)
            out[step] = (x.copy(), e, nhc.T if nhc is not None else 0.0, v.copy())
    return out
