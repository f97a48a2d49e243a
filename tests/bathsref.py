"""The masked host loops of the several-bath tests (tests/test_bathsref.py, tests/test_gpu_langevin_baths.py): velocity
Verlet on a group of atoms with a LIST of Langevin thermostats, each on a group of its own -- LAMMPS `fix nve` next to
several `fix langevin` on disjoint groups -- around tests/langevinref.py as it is.  Bath k is a pair
(langevinref.Langevin, group): its force, its `zero` mean (over its group's count) and its tally run over its group alone.
With one bath every loop here is groupref's bit for bit (tests/test_bathsref.py).  A helper module, not a test module; no GPU."""
from __future__ import annotations

import numpy as np

from lammps_plugins_amd.host import system as S
import groupref

ALL_BIT, INTEGRATE_BIT = groupref.ALL_BIT, groupref.INTEGRATE_BIT
BATH_BITS = (4, 8, 16)


def masks(s):
    """(mask by TAG [n + 1], integrate group, [bath A, B, C]) as boolean arrays in the order of s.  Bit 1 on every atom;
    the integrate group (bit 2) is groupref.masks': everything but a z-slab of about a third of the cell and the tags
    divisible by 5.  The baths lie inside it and mix tag-modulus classes with slabs along x:
      A (bit 4)  tag % 4 == 0 in the half x >= 1/2
      B (bit 8)  tag % 4 == 1 in the half x >= 1/2
      C (bit 16) tag % 4 == 2 in the half x >= 1/2 and tag % 4 == 3 in the quarter x >= 3/4
    so between x = 1/2 and 3/4 neighbouring atoms -- lanes of one wave -- belong to all three baths, to none (tag % 4 == 3)
    and to the held atoms.  The half x < 1/2 holds no bath atom: the device's curve runs through it first, so whole
    256-atom blocks of it do the integrator's work alone."""
    lam = s.box.x2lamda(S.wrap(s.box, s.x))
    g = ~(lam[:, 2] < 1.0 / 3.0) & (s.tag % 5 != 0)
    right = g & (lam[:, 0] >= 0.5)
    baths = [right & (s.tag % 4 == 0),
             right & (s.tag % 4 == 1),
             right & ((s.tag % 4 == 2) | ((s.tag % 4 == 3) & (lam[:, 0] >= 0.75)))]
    by_tag = np.zeros(int(s.tag.max()) + 1, dtype=np.int32)
    m = ALL_BIT | np.where(g, INTEGRATE_BIT, 0)
    for bit, b in zip(BATH_BITS, baths):
        m = m | np.where(b, bit, 0)
    by_tag[s.tag] = m
    return by_tag, g, baths


BATH_BITS4 = BATH_BITS + (32,)


def masks4(s):
    """masks() with a fourth bath D (bit 32) cut out of what the three leave unthermostatted, for the fourth slot of the
    baths and of the heat sources; A, B, C, the integrate group and the held atoms are those of masks():
      D (bit 32) two of every three atoms with tag % 4 == 3 between x = 1/2 and 3/4 (counted in the order of s), and the
                 even tags between x = 1/4 and 1/2
    Between x = 1/2 and 3/4 a wave then holds atoms of all four baths, of none (the third atoms) and held atoms; the quarter
    x < 1/4 and the odd tags of the second quarter stay integrated and unthermostatted."""
    by_tag, g, baths = masks(s)
    lam = s.box.x2lamda(S.wrap(s.box, s.x))
    x = lam[:, 0]
    zone = g & (s.tag % 4 == 3) & (x >= 0.5) & (x < 0.75)
    d = (zone & (np.cumsum(zone) % 3 != 0)) | (g & (s.tag % 2 == 0) & (x >= 0.25) & (x < 0.5))
    by_tag = by_tag.copy()
    by_tag[s.tag] |= np.where(d, BATH_BITS4[3], 0).astype(np.int32)
    return by_tag, g, baths + [d]


def check_masks(s, g, baths):
    """the conditions on the input every several-bath test states before anything is launched"""
    any_bath = np.zeros(s.n, dtype=bool)
    for k, b in enumerate(baths):
        assert 0.05 * s.n <= b.sum() <= 0.40 * s.n, (k, int(b.sum()), s.n)
        assert not (b & ~g).any(), k                       # inside the integrate group
        assert not (b & any_bath).any(), k                 # pairwise disjoint
        any_bath |= b
    assert (g & ~any_bath).sum() >= 0.10 * s.n, (int((g & ~any_bath).sum()), s.n)   # integrated, unthermostatted
    assert (~g).sum() >= 0.25 * s.n, (int((~g).sum()), s.n)                          # held


def baths_force(baths, n, tag, type_, v, phase=0):
    """the Langevin force of step n on every atom: bath k's on its group (groupref.lgv_force), nothing elsewhere"""
    fl = np.zeros_like(v)
    for lgv, l in baths:
        l = np.asarray(l, dtype=bool)
        fl[l] = lgv.force(n, tag[l], type_[l], v[l], phase=phase)
    return fl


def run_langevin(x, v, mass_atom, tag, type_, force, baths, first, last, ftm2v, group, on_step=None):
    """groupref.run_langevin with a list of (Langevin, group) pairs instead of one thermostat and its group"""
    dt = baths[0][0].dt
    dtf = 0.5 * dt * ftm2v
    g = np.asarray(group, dtype=bool)
    m = mass_atom[g][:, None]
    for lgv, _ in baths:
        lgv.setup(first, last)
    f, pe = force(x)
    f = f + baths_force(baths, first, tag, type_, v, phase=1)
    for lgv, l in baths:
        lgv.tally_setup(v[l])
    for n in range(first + 1, last + 1):
        v[g] += dtf * f[g] / m
        x[g] += dt * v[g]
        f, pe = force(x)
        f = f + baths_force(baths, n, tag, type_, v)
        v[g] += dtf * f[g] / m
        for lgv, l in baths:
            lgv.tally_step(v[l])
        if on_step is not None:
            on_step(n, x, v, pe)
    return x, v


def host_baths(make_engine, s, v0, nsteps, every, rebuild_every, group, baths, dt=0.001):
    """groupref.host_group with the baths: velocity Verlet on `group` around the oracle, the lists built anew every
    rebuild_every steps; {step: (x by tag, [tally of bath k], v by tag)} for the steps in `every`"""
    g = np.asarray(group, dtype=bool)
    mg = s.mass[s.type][g]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
    for lgv, _ in baths:
        lgv.setup(0, nsteps)
    f = f + baths_force(baths, 0, s.tag, s.type, v, phase=1)
    for lgv, l in baths:
        lgv.tally_setup(v[l])
    dtf = 0.5 * dt * S.FTM2V
    out = {}
    for step in range(1, nsteps + 1):
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
        f = f + baths_force(baths, step, s.tag, s.type, v)
        v[g] += dtf * f[g] / mg[:, None]
        for lgv, l in baths:
            lgv.tally_step(v[l])
        if step in every:
            out[step] = (x.copy(), [lgv.scalar() for lgv, _ in baths], v.copy())
    return out
