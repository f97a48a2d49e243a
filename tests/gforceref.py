"""The host reference of the prescribed group forces (tests/test_gforceref.py, tests/test_gpu_gforce_mdp.py): LAMMPS fix
setforce, fix addforce and fix aveforce with constant values, restated from their documentation as one sequential rule --
the fixes act one after the other, in the order of their definition, each on the forces as the one before left them -- and
the masked velocity-Verlet loop of tests/springref.py::host_spring around the oracle forces with them applied after every
force evaluation, the setup's included.  A slot is a dict
    dict(kind="set" | "add" | "ave", f=(fx, fy, fz) with None for NULL, group=<boolean array or None: every atom>)
and with g the forces as the slots before k left them, over the atoms of its group
    set:  F_k = sum g;                              then g[d] = f[d] where f[d] is not None
    add:  F_k = sum g,  E_k = -sum f . xu  (xu = x + h . image);   then g += f
    ave:  F_k = sum g,  N_k = the atoms;            then g[d] = F_k[d] / N_k + f[d] where f[d] is not None (N_k > 0)
F_k is LAMMPS' f_ID[1..3] of all three styles, E_k the f_ID of addforce.
post_force is that rule as written.  walk is what a device lane does: one atom's slots in order on its own running force, the
group sums gathered on the way -- the same thing whenever no slot shares atoms with an "ave" in front of it
(shares_with_ave_in_front), which is what the device's set-up refuses.
A helper module, not a test module; no GPU."""
from __future__ import annotations

import math

import numpy as np

from lammps_plugins_amd.host import system as S
import bathsref
import indentref
import springref

# What the device may differ by in F_k and E_k (tests/test_gpu_gforce_mdp.py): 100 times what the reference itself moves by
# when every slot's atoms are summed in a random order and with math.fsum, rounded up in the second digit
# (tests/test_gforceref.py measures it and asserts the factor; the GPU test's docstring holds the measured values)
F_TOL, E_TOL = 1.4e-10, 5.7e-11


def used(sl):
    return np.array([a is not None for a in sl["f"]])


def values(sl):
    return np.array([0.0 if a is None else float(a) for a in sl["f"]])


def members(sl, n):
    return np.arange(n) if sl.get("group") is None else np.flatnonzero(np.asarray(sl["group"], dtype=bool))


def _total(rows, exact):
    """the sum of the rows of [m][c]: one after the other in the given order, or math.fsum"""
    if len(rows) == 0:
        return np.zeros(rows.shape[1])
    if exact:
        return np.array([math.fsum(rows[:, c]) for c in range(rows.shape[1])])
    return np.cumsum(rows, axis=0)[-1]


def shares_with_ave_in_front(slots, n):
    """[(j, k, atoms)] for every slot k that shares atoms with an "ave" slot j in front of it"""
    out = []
    for k, sk in enumerate(slots):
        for j in range(k):
            if slots[j]["kind"] != "ave":
                continue
            both = len(np.intersect1d(members(slots[j], n), members(sk, n)))
            if both:
                out.append((j, k, both))
    return out


def post_force(slots, box, x, img, f, orders=None, exact=False):
    """the fixes' post_force, slot after slot, on f in place; per slot dict(energy, ftotal [3], atoms, value [3]: what it
    wrote or added per dimension, 0 where NULL).  orders: per slot a permutation of ALL atoms to sum its group in; exact:
    math.fsum instead of one atom after the other"""
    xu = springref.unwrap(box, x, img)
    out = []
    for k, sl in enumerate(slots):
        idx = members(sl, len(f))
        if orders is not None and orders[k] is not None:
            idx = idx[np.argsort(np.asarray(orders[k])[idx], kind="stable")]
        use, val = used(sl), values(sl)
        F = _total(f[idx], exact)
        E = 0.0
        if sl["kind"] == "set":
            f[np.ix_(idx, np.flatnonzero(use))] = val[use]
        elif sl["kind"] == "add":
            assert use.all(), "addforce takes three numbers"
            E = -float(_total((xu[idx] @ val)[:, None], exact)[0])
            f[idx] += val
        elif sl["kind"] == "ave":
            val = np.where(use, F / len(idx) + val, 0.0) if len(idx) else np.zeros(3)
            if len(idx):
                f[np.ix_(idx, np.flatnonzero(use))] = val[use]
        else:
            raise KeyError(sl["kind"])
        out.append(dict(energy=E, ftotal=F, atoms=int(len(idx)), value=np.where(use, val, 0.0)))
    return out


def walk(slots, box, x, img, f):
    """the same, one atom at a time as a device lane does it: the atom's slots in order on its running force, which ends at
    an "ave" slot (nothing behind it holds the atom); then the averages from the gathered sums, and every atom again.
    Returns (the new forces, states as post_force's)"""
    n = len(f)
    assert not shares_with_ave_in_front(slots, n)
    xu = springref.unwrap(box, x, img)
    inside = np.zeros((len(slots), n), dtype=bool)
    for k, sl in enumerate(slots):
        inside[k, members(sl, n)] = True
    F = np.zeros((len(slots), 3))
    E = np.zeros(len(slots))
    N = inside.sum(axis=1)

    def one(i, aves):
        g = f[i].copy()
        for k, sl in enumerate(slots):
            if not inside[k, i]:
                continue
            use, val = used(sl), values(sl)
            if aves is None:
                F[k] += g
            if sl["kind"] == "set":
                g[use] = val[use]
            elif sl["kind"] == "add":
                if aves is None:
                    E[k] -= float(val @ xu[i])
                g += val
            elif aves is not None:
                g[use] = aves[k][use]
        return g
    for i in range(n):
        one(i, None)
    aves = [F[k] / N[k] + values(sl) if sl["kind"] == "ave" and N[k] else None for k, sl in enumerate(slots)]
    out = np.array([one(i, aves) for i in range(n)]).reshape(n, 3)
    states = []
    for k, sl in enumerate(slots):
        val = values(sl) if sl["kind"] != "ave" else (aves[k] if N[k] else np.zeros(3))
        states.append(dict(energy=float(E[k]), ftotal=F[k].copy(), atoms=int(N[k]), value=np.where(used(sl), val, 0.0)))
    return out, states


def host_gforce(make_engine, s, v0, img0, nsteps, every, rebuild_every, group, slots, dt=0.001, orders=None, exact=False, cut=None,
                baths=None, inds=None, springs=None, skin=None):
    """springref.host_spring with the group forces: velocity Verlet on `group` around the oracle, the lists built anew every
    rebuild_every steps -- where the atoms are wrapped and their image flags (img0 [n][3] counts, in the order of s) take up
    the box vectors -- and after every force evaluation the indenters `inds` (indentref.post_force), the springs `springs`
    (springref.post_force), the slots (post_force, above) and last the Langevin forces of `baths` (bathsref.baths_force): the
    order of the device, whose kick adds the bath's force to what the stages left.
    {step: (x by tag, [state of slot k], v by tag)} for the steps in `every` and for step 0 (the setup), and
    dict(fmax: per slot the largest |F_k| over ALL steps, flagged: atoms of `group` whose image flag changed).
    cut = k: the host starts a second run behind step k (a new setup: the forces are computed anew, from the same positions;
    the indenters' centres and the springs' tether points start again);
    skin: assert that no atom has moved more than half of it since the last build (heatref.host_heat's rule: a prescribed
    force can drive atoms faster than the fixed interval allows for, and the reference's list must not go stale unseen)"""
    g = np.asarray(group, dtype=bool)
    m = s.mass[s.type]
    mg = m[g]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    img = np.array(img0, dtype=np.int64, copy=True)
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    x_built = x.copy()
    fmax = [0.0] * len(slots)

    def forces(step, n, phase=0, with_baths=True):
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"].copy()
        if inds:
            indentref.post_force(inds, n, 0, dt, s.box, x, f)
        if springs:
            springref.post_force(springs, n, 0, dt, s.box, x, img, m, f)
        st = post_force(slots, s.box, x, img, f, orders=orders, exact=exact)
        if baths and with_baths:
            f += bathsref.baths_force(baths, step, s.tag, s.type, v, phase=phase)
        for k, q in enumerate(st):
            fmax[k] = max(fmax[k], float(np.abs(q["ftotal"]).max()))
        return f, st
    if baths:
        for lgv, _ in baths:
            lgv.setup(0, nsteps)
    f, st = forces(0, 0, phase=1)
    dtf = 0.5 * dt * S.FTM2V
    out = {0: (x.copy(), st, v.copy())}
    base = 0
    for step in range(1, nsteps + 1):
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        if step % rebuild_every == 0:
            img += np.floor(s.box.x2lamda(x)).astype(np.int64)
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
            x_built = x.copy()
        elif skin is not None:
            far = float(np.sqrt(((x - x_built) ** 2).sum(axis=1)).max())
            assert far <= 0.5 * skin, f"the reference's own list is stale at step {step}: an atom moved {far:.3f} A"
        f, st = forces(step, step - base)
        v[g] += dtf * f[g] / mg[:, None]
        if step in every:
            out[step] = (x.copy(), st, v.copy())
        if cut is not None and step == cut:
            base = step
            f, st = forces(step, 0, with_baths=False)
    flagged = int(((img != np.asarray(img0)).any(axis=1) & g).sum())
    return out, dict(fmax=fmax, flagged=flagged)
