"""The host reference of the tether springs (tests/test_springref.py, tests/test_gpu_spring_mdp.py): LAMMPS fix spring tether
restated from its documentation -- a spring of stiffness K and rest length R0 between the centre of mass of a group, taken
over the unwrapped positions, and a tether point; a dimension given as NULL takes no part -- with the one extension of the
device library, a tether point that moves at a constant velocity, and the masked velocity-Verlet loop of
tests/indentref.py::host_indent around the oracle forces with the spring forces added after every force evaluation, the
setup's included.  A spring is a dict
    dict(k=, r0=, c=(x, y, z) with None for NULL, vel=(vx, vy, vz), group=<boolean array or None: every atom>)
        M = sum m_i,  xcm = (sum m_i xu_i) / M,  d = xcm - p (NULL dimensions zeroed),  r = max(|d|, 1e-10),  dr = r - R0
        F = K d dr / r,  E = K dr^2 / 2,  f_i -= (F / M) m_i,  ftotal = (-Fx, -Fy, -Fz, sign(dr) |F|)
A helper module, not a test module; no GPU."""
from __future__ import annotations

import math

import numpy as np

from lammps_plugins_amd.host import system as S
import bathsref
import indentref

RMIN = 1.0e-10


def used(sp):
    return np.array([a is not None for a in sp["c"]])


def tether(sp, n, first, dt):
    """the tether point that belongs to the forces of step n of a run that began at step `first`; 0 in a NULL dimension"""
    c = np.array([0.0 if a is None else float(a) for a in sp["c"]])
    vel = np.asarray(sp.get("vel", (0.0, 0.0, 0.0)), dtype=float)
    return np.where(used(sp), c + vel * ((n - first) * dt), 0.0)


def unwrap(box, x, img):
    """x + h . image: the positions the centre of mass is taken over"""
    return np.asarray(x, dtype=float) + S.mul_upper(np.asarray(img, dtype=float), box.h)


def spring_tether(sp, p, m, xu, order=None, exact=False):
    """one spring with its tether point at p: dict(energy, ftotal [4], xcm, tether, mass, atoms, fm: F / M [3], dr).
    order: a permutation of ALL atoms to sum the group's m xu in; exact: math.fsum instead of one atom after the other.  M is
    math.fsum of the masses throughout"""
    idx = np.arange(len(m)) if sp.get("group") is None else np.flatnonzero(np.asarray(sp["group"], dtype=bool))
    if order is not None:
        idx = idx[np.argsort(np.asarray(order)[idx], kind="stable")]
    if len(idx) == 0:                           # (a group that lost its atoms to a new mask: no centre of mass, no force)
        return dict(energy=0.0, ftotal=np.zeros(4), xcm=np.zeros(3), tether=np.asarray(p, dtype=float), mass=0.0, atoms=0,
                    fm=np.zeros(3), dr=0.0)
    mi = np.asarray(m, dtype=float)[idx]
    mx = mi[:, None] * np.asarray(xu, dtype=float)[idx]
    M = math.fsum(mi)                           # (the sum of the masses is exact in every mode: it has one value)
    if exact:
        sx = np.array([math.fsum(mx[:, c]) for c in range(3)])
    else:
        sx = np.cumsum(mx, axis=0)[-1]         # (one atom after the other, in the given order)
    xcm = sx / M
    d = np.where(used(sp), xcm - p, 0.0)
    r = max(math.sqrt(float((d * d).sum())), RMIN)
    dr = r - sp.get("r0", 0.0)
    F = sp["k"] * d * dr / r
    fmag = math.sqrt(float((F * F).sum()))
    return dict(energy=0.5 * sp["k"] * dr * dr, ftotal=np.array([-F[0], -F[1], -F[2], -fmag if dr < 0.0 else fmag]), xcm=xcm,
                tether=np.asarray(p, dtype=float), mass=M, atoms=int(len(idx)), fm=F / M, dr=dr)


def post_force(springs, n, first, dt, box, x, img, m, f=None, orders=None, exact=False):
    """FixSpring::post_force of every spring for the forces of step n: takes (F / M) m_i off f (if given), spring after
    spring, and returns the state of each"""
    xu = unwrap(box, x, img)
    out = []
    for k, sp in enumerate(springs):
        st = spring_tether(sp, tether(sp, n, first, dt), m, xu, order=None if orders is None else orders[k], exact=exact)
        if f is not None:
            g = slice(None) if sp.get("group") is None else np.asarray(sp["group"], dtype=bool)
            f[g] -= st["fm"][None, :] * np.asarray(m, dtype=float)[g][:, None]
        out.append(st)
    return out


def run(x, v, m, force, springs, first, last, dt, ftm2v, group, box, img=None, on_step=None):
    """velocity Verlet on `group` with the springs, steps first + 1 .. last, in place, without wrapping (the image flags
    stay what they are): force(x) -> (f, pe); on_step(n, x, v, pe, states)"""
    dtf = 0.5 * dt * ftm2v
    g = np.asarray(group, dtype=bool)
    mg = m[g][:, None]
    img = np.zeros((len(m), 3), dtype=np.int64) if img is None else img
    f, pe = force(x)
    f = f.copy()
    st = post_force(springs, first, first, dt, box, x, img, m, f)
    if on_step is not None:
        on_step(first, x, v, pe, st)
    for n in range(first + 1, last + 1):
        v[g] += dtf * f[g] / mg
        x[g] += dt * v[g]
        f, pe = force(x)
        f = f.copy()
        st = post_force(springs, n, first, dt, box, x, img, m, f)
        v[g] += dtf * f[g] / mg
        if on_step is not None:
            on_step(n, x, v, pe, st)
    return x, v


def host_spring(make_engine, s, v0, img0, nsteps, every, rebuild_every, group, springs, dt=0.001, first=0, orders=None,
                exact=False, cut=None, baths=None, inds=None, ind_orders=None, dforce=0.0, regroup=None, skin=None, on_force=None,
                periodic=(True, True, True), keep_held=False):
    """indentref.host_indent with the springs: velocity Verlet on `group` around the oracle, the lists built anew every
    rebuild_every steps -- where the atoms are wrapped and their image flags (img0 [n][3] counts, by the order of s, at the
    start) take up the box vectors -- and FixSpring::post_force after every force evaluation, behind the Langevin forces of
    `baths` (bathsref.host_baths) and the indenters `inds` (indentref.post_force) if there are any.
    {step: (x by tag, [state of spring k], v by tag, xu by tag, [state of indenter k])} for the steps in `every` and for step
    0 (the setup), and dict(fmax: per spring the largest |F| over ALL steps, flagged: atoms of `group` whose image flag
    changed during the run).
    cut = k: the host starts a second run behind step k (mdp_spring_run(first + k), mdp_indent_run(first + k) and a new
    setup): the tether points and the centres start again at c and the forces are computed anew, from the same positions.
    The nets' extensions (tests/nets.py, the `postforce` net) -- `springs` may be empty, the indenters alone:
    ind_orders: per indenter a permutation its touching atoms are summed in (indentref.post_force);
    dforce: every component of the oracle's forces of every step gets an error drawn uniformly from +-dforce;
    regroup = {step: (springs, inds)}: behind the read of that step the host sets a new mask -- from the forces of the next
    step on these lists, with their groups, stand for the old ones (a spring whose group is empty reports zeros);
    skin: assert that no atom has moved more than half of it since the last build (heatref.host_heat's rule);
    on_force(step, x, img, spring states, indenter states): called behind every force evaluation of a step (0: the setup);
    periodic: what the indenters' minimum image takes per dimension;
    keep_held: a list build leaves the atoms outside `group` where they are, bit for bit, as a host that wraps only the atoms
    that left the box does (S.wrap writes every atom anew, which moves an atom of a sheared box by an ulp)."""
    g = np.asarray(group, dtype=bool)
    m = s.mass[s.type]
    mg = m[g]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    img = np.array(img0, dtype=np.int64, copy=True)
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    x_built = x.copy()
    cur = dict(springs=springs, inds=inds or [])
    noise = np.random.default_rng(20261) if dforce else None

    def forces(step, n, phase=0, with_baths=True):
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"].copy()
        if dforce:
            f += noise.uniform(-dforce, dforce, f.shape)
        if baths and with_baths:
            f += bathsref.baths_force(baths, step, s.tag, s.type, v, phase=phase)
        ist = indentref.post_force(cur["inds"], n, first, dt, s.box, x, f, periodic=periodic, orders=ind_orders) if cur["inds"] else []
        return f, post_force(cur["springs"], n, first, dt, s.box, x, img, m, f, orders=orders, exact=exact), ist
    if baths:
        for lgv, _ in baths:
            lgv.setup(0, nsteps)
    f, st, ist = forces(0, first, phase=1)
    dtf = 0.5 * dt * S.FTM2V
    fmax = [0.0] * len(springs)

    def note(step, st, ist):
        for k, q in enumerate(st):
            fmax[k] = max(fmax[k], abs(float(q["ftotal"][3])))
        if on_force is not None:
            on_force(step, x, img, st, ist)

    def read():
        return (x.copy(), st, v.copy(), unwrap(s.box, x, img), ist)
    note(0, st, ist)
    out = {0: read()}
    base = 0
    for step in range(1, nsteps + 1):
        v[g] += dtf * f[g] / mg[:, None]
        x[g] += dt * v[g]
        if step % rebuild_every == 0:
            img += np.floor(s.box.x2lamda(x)).astype(np.int64)
            xw = S.wrap(s.box, x)
            if keep_held:
                xw[~g] = x[~g]
            x = xw
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
            x_built = x.copy()
        elif skin is not None:
            far = float(np.sqrt(((x - x_built) ** 2).sum(axis=1)).max())
            assert far <= 0.5 * skin, f"the reference's own list is stale at step {step}: an atom moved {far:.3f} A"
        f, st, ist = forces(step, first + step - base)
        note(step, st, ist)
        v[g] += dtf * f[g] / mg[:, None]
        if step in every:
            out[step] = read()
        if regroup is not None and step in regroup:
            cur["springs"], cur["inds"] = regroup[step]
        if cut is not None and step == cut:      # the second run's setup: same positions, tether points and centres at c again
            base = step
            f, st, ist = forces(step, first, with_baths=False)
            note(step, st, ist)
    flagged = int(((img != np.asarray(img0)).any(axis=1) & g).sum())
    return out, dict(fmax=fmax, flagged=flagged)
