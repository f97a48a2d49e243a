"""The host reference of the indenters (tests/test_indentref.py, tests/test_gpu_indent_mdp.py): LAMMPS FixIndent::post_force
with `units box` restated from its documentation -- sphere, cylinder and plane, both sides, Domain::minimum_image for
orthogonal and tilted boxes, and a centre that moves as vdisplace(c, vel) -- and the masked velocity-Verlet loop of
tests/heatref.py / tests/bathsref.py around the oracle forces with the indenter forces added after every force evaluation,
the setup's included.  An indenter is a dict
    dict(shape="sphere" | "cylinder" | "plane", k=, r=, c=(x, y, z), dim=0 | 1 | 2, side="out" | "in" | "lo" | "hi",
         vel=(vx, vy, vz), group=<boolean array or None: every atom>)
A helper module, not a test module; no GPU."""
from __future__ import annotations

import math

import numpy as np

from lammps_plugins_amd.host import system as S
import bathsref


def centre(ind, n, first, dt):
    """the centre that belongs to the forces of step n of a run that began at step `first`: vdisplace(c, vel)"""
    return np.asarray(ind["c"], dtype=float) + np.asarray(ind.get("vel", (0.0, 0.0, 0.0)), dtype=float) * ((n - first) * dt)


def minimum_image(box, d, periodic=(True, True, True), taken=None):
    """Domain::minimum_image on the rows of d: one wrap per periodic dimension, z then y then x; a wrap in z carries
    (xz, yz), a wrap in y carries xy.  taken: a dict that receives, per periodic dimension 0 | 1 | 2, the sign of the
    wrap every row took there (0: none)"""
    d = np.array(d, dtype=float, copy=True).reshape(-1, 3)
    xprd, yprd, zprd = box.prd
    xy, xz, yz = box.tilt
    if periodic[2]:
        s = np.where(np.abs(d[:, 2]) > 0.5 * zprd, np.where(d[:, 2] < 0.0, 1.0, -1.0), 0.0)
        d[:, 2] += s * zprd
        d[:, 1] += s * yz
        d[:, 0] += s * xz
        if taken is not None:
            taken[2] = s
    if periodic[1]:
        s = np.where(np.abs(d[:, 1]) > 0.5 * yprd, np.where(d[:, 1] < 0.0, 1.0, -1.0), 0.0)
        d[:, 1] += s * yprd
        d[:, 0] += s * xy
        if taken is not None:
            taken[1] = s
    if periodic[0]:
        s = np.where(np.abs(d[:, 0]) > 0.5 * xprd, np.where(d[:, 0] < 0.0, 1.0, -1.0), 0.0)
        d[:, 0] += s * xprd
        if taken is not None:
            taken[0] = s
    return d


def depth(ind, ctr, box, x, periodic=(True, True, True), taken=None):
    """(dr, unit vector the force on a touching atom points along, r) of every atom for the indenter centred at ctr;
    taken: as minimum_image takes it (a plane takes no minimum image and leaves it empty)"""
    x = np.asarray(x, dtype=float).reshape(-1, 3)
    side = ind.get("side", "out")
    dim = int(ind.get("dim", 0))
    if ind["shape"] == "plane":
        u = np.zeros_like(x)
        if side == "lo":
            dr = x[:, dim] - ctr[dim]
            u[:, dim] = 1.0
        else:
            dr = ctr[dim] - x[:, dim]
            u[:, dim] = -1.0
        return dr, u, np.abs(dr)
    d = x - ctr
    if ind["shape"] == "cylinder":
        d[:, dim] = 0.0
    d = minimum_image(box, d, periodic, taken)
    r = np.sqrt((d * d).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(r[:, None] > 0.0, d / r[:, None], 0.0)
    if side == "in":
        return ind["r"] - r, -u, r
    return r - ind["r"], u, r


def terms(ind, ctr, box, x, periodic=(True, True, True)):
    """per atom: (force [n][3], energy [n], in contact [n]) of one indenter, its group applied"""
    dr, u, r = depth(ind, ctr, box, x, periodic)
    on = dr < 0.0
    if ind.get("group") is not None:
        on &= np.asarray(ind["group"], dtype=bool)
    f = np.where(on[:, None], (ind["k"] * dr * dr)[:, None] * u, 0.0)
    e = np.where(on, -(ind["k"] / 3.0) * dr * dr * dr, 0.0)
    return f, e, on


def post_force(inds, n, first, dt, box, x, f=None, periodic=(True, True, True), orders=None, exact=False):
    """FixIndent::post_force of every indenter for the forces of step n: adds into f (if given) and returns per indenter
    dict(energy, force on the indenter [3], contacts, centre, fmax: the largest force on one atom, deepest: the largest
    -dr, terms: sum of the magnitudes of the energy terms and of the force terms per component).  orders: per indenter a
    permutation of its touching atoms to sum them in; exact: math.fsum instead of numpy's sum"""
    out = []
    for k, ind in enumerate(inds):
        ctr = centre(ind, n, first, dt)
        fk, ek, on = terms(ind, ctr, box, x, periodic)
        if f is not None:
            f += fk
        idx = np.flatnonzero(on)
        if orders is not None and orders[k] is not None:
            idx = idx[np.argsort(orders[k][idx], kind="stable")]
        if exact:
            e = math.fsum(ek[idx])
            fi = -np.array([math.fsum(fk[idx, c]) for c in range(3)])
        else:
            e, fi = 0.0, np.zeros(3)
            for i in idx:               # (in the given order, one atom at a time)
                e += ek[i]
                fi -= fk[i]
        dr = depth(ind, ctr, box, x, periodic)[0]
        out.append(dict(energy=float(e), force=fi, contacts=int(len(idx)), centre=ctr,
                        fmax=float(np.sqrt((fk * fk).sum(axis=1)).max()) if len(idx) else 0.0,
                        deepest=float(-dr[idx].min()) if len(idx) else 0.0,
                        terms=(float(np.abs(ek[idx]).sum()), np.abs(fk[idx]).sum(axis=0))))
    return out


def run(x, v, m, force, inds, first, last, dt, ftm2v, group, box, on_step=None):
    """velocity Verlet on `group` with the indenters, steps first + 1 .. last, in place: force(x) -> (f, pe);
    on_step(n, x, v, pe, states)"""
    dtf = 0.5 * dt * ftm2v
    g = np.asarray(group, dtype=bool)
    mg = m[g][:, None]
    f, pe = force(x)
    f = f.copy()
    st = post_force(inds, first, first, dt, box, x, f)
    if on_step is not None:
        on_step(first, x, v, pe, st)
    for n in range(first + 1, last + 1):
        v[g] += dtf * f[g] / mg
        x[g] += dt * v[g]
        f, pe = force(x)
        f = f.copy()
        st = post_force(inds, n, first, dt, box, x, f)
        v[g] += dtf * f[g] / mg
        if on_step is not None:
            on_step(n, x, v, pe, st)
    return x, v


def host_indent(make_engine, s, v0, nsteps, every, rebuild_every, group, inds, dt=0.001, first=0, orders=None, cut=None,
                baths=None, energies=False):
    """groupref.host_group with the indenters: velocity Verlet on `group` around the oracle, the lists built anew every
    rebuild_every steps, FixIndent::post_force after every force evaluation.
    {step: (x by tag, [state of indenter k, as post_force gives it], v by tag)} for the steps in `every` and for step 0 (the
    setup), and dict(fmax, deepest) over ALL steps.
    cut = k: the host starts a second run behind step k (mdp_indent_run(first + k) and a new setup): the centres start again
    at c and the forces are computed anew, from the same positions.
    baths: a list of (langevinref.Langevin, group) as bathsref.host_baths takes them, next to the indenters.
    energies: a fourth entry per read, (KE of the group's atoms, E_pair)"""
    g = np.asarray(group, dtype=bool)
    mg = s.mass[s.type][g]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    r = eng.compute(x, eflag=1, vflag=0)
    f = r["f_owned"].copy()
    if baths:
        for lgv, _ in baths:
            lgv.setup(0, nsteps)
        f += bathsref.baths_force(baths, 0, s.tag, s.type, v, phase=1)
    st = post_force(inds, first, first, dt, s.box, x, f, orders=orders)
    dtf = 0.5 * dt * S.FTM2V
    worst = dict(fmax=0.0, deepest=0.0)

    def note(st):
        for q in st:
            worst["fmax"] = max(worst["fmax"], q["fmax"])
            worst["deepest"] = max(worst["deepest"], q["deepest"])

    def read(r):
        ke = 0.5 * S.MVV2E * float((s.mass[s.type][:, None] * v * v).sum())
        return (x.copy(), st, v.copy()) + (((ke, float(r["eng"])),) if energies else ())
    note(st)
    out = {0: read(r)}
    base = 0
    for step in range(1, nsteps + 1):
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
        r = eng.compute(x, eflag=1, vflag=0)
        f = r["f_owned"].copy()
        if baths:
            f += bathsref.baths_force(baths, step, s.tag, s.type, v)
        st = post_force(inds, first + step - base, first, dt, s.box, x, f, orders=orders)
        note(st)
        v[g] += dtf * f[g] / mg[:, None]
        if step in every:
            out[step] = read(r)
        if cut is not None and step == cut:      # the second run's setup: same positions, the centres at c again
            base = step
            f = eng.compute(x, eflag=1, vflag=0)["f_owned"].copy()
            st = post_force(inds, first, first, dt, s.box, x, f, orders=orders)
            note(st)
    return out, worst
