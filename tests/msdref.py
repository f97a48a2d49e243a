"""NumPy reference of the image flags and of compute msd (tests only): velocity Verlet around the oracle (mdref.RebomosCPU /
AeamCPU, or any engine with compute(x)["f_owned"]) that keeps a WRAPPED x and an integer image per atom, as LAMMPS does --
Domain::remap at every list build, on the steps the device run is forced to build on -- and forms the unwrapped positions
x + h . image and the four values of compute msd with math.fsum.  A helper module, not a test module; no GPU."""
from __future__ import annotations

import math

import numpy as np

from lammps_plugins_amd.host import system as S


def remap(box: S.Box, x, image, periodic=(1, 1, 1)):
    """Domain::remap: atoms outside the periodic box come back by whole box vectors, which their image counts; atoms
    inside keep their coordinates bit for bit.  Returns (x, image), new arrays."""
    lam = box.x2lamda(x)
    s = np.floor(lam)
    rest = lam - s
    s[rest >= 1.0] += 1.0            # (a tiny negative lamda: lam - floor(lam) rounds to 1)
    s *= np.asarray(periodic, dtype=np.float64)
    moved = np.any(s != 0.0, axis=1)
    x = np.array(x, dtype=np.float64, copy=True)
    x[moved] -= S.mul_upper(s[moved], box.h)
    return x, np.asarray(image, dtype=np.int64) + s.astype(np.int64)


def unwrap(box: S.Box, x, image):
    """xu = x + h . image: xu_x = x + xprd ix + xy iy + xz iz, xu_y = y + yprd iy + yz iz, xu_z = z + zprd iz"""
    return np.asarray(x, dtype=np.float64) + S.mul_upper(np.asarray(image, dtype=np.float64), box.h)


def centre_of_mass(xu, mass_per_atom):
    m = np.asarray(mass_per_atom, dtype=np.float64)
    tot = math.fsum(m)
    return np.array([math.fsum(m * xu[:, d]) / tot for d in range(3)])


def msd_values(xu, xu0, sel=None, mass_per_atom=None, com=False):
    """LAMMPS compute msd: the means over the selected atoms of dx^2, dy^2, dz^2, and their total; com: with the
    displacement of the selection's centre of mass taken out.  Sums with math.fsum."""
    sel = np.ones(len(xu), dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    a, b = np.asarray(xu)[sel], np.asarray(xu0)[sel]
    d = a - b
    if com:
        m = np.asarray(mass_per_atom)[sel]
        d = d - (centre_of_mass(a, m) - centre_of_mass(b, m))
    v = [math.fsum(d[:, k] * d[:, k]) / len(d) for k in range(3)]
    return np.array(v + [v[0] + v[1] + v[2]])


def run(make_engine, s: S.System, v0, nsteps, rebuild_every, reads, dt=0.001, periodic=(1, 1, 1)):
    """velocity Verlet from the wrapped positions of `s` with every image 0; lists, ghosts and the remap anew on every
    step that is a multiple of rebuild_every (Verlet::run order: initial half, remap + build, force, final half).
    {step in reads: (x wrapped, image counts, xu, v)} by tag order of `s`, and step 0."""
    m = s.mass[s.type][:, None]
    x = S.wrap(s.box, s.x)
    image = np.zeros((s.n, 3), dtype=np.int64)
    v = np.array(v0, dtype=np.float64, copy=True)
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    f = eng.compute(x, eflag=0, vflag=0)["f_owned"]
    dtf = 0.5 * dt * S.FTM2V
    out = {0: (x.copy(), image.copy(), unwrap(s.box, x, image), v.copy())}
    for step in range(1, nsteps + 1):
        v += dtf * f / m
        x += dt * v
        if step % rebuild_every == 0:
            x, image = remap(s.box, x, image, periodic)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
        f = eng.compute(x, eflag=0, vflag=0)["f_owned"]
        v += dtf * f / m
        if step in reads:
            out[step] = (x.copy(), image.copy(), unwrap(s.box, x, image), v.copy())
    return out


class FreeFlight:
    """an engine without forces: the atoms fly straight (the rigid drift of tests/test_msdref.py)"""

    def __init__(self, s):
        self.n = s.n

    def compute(self, x, eflag=0, vflag=0):
        return {"f_owned": np.zeros((self.n, 3)), "eng": 0.0}


# ---- the drift cases of tests/test_gpu_msd_mdp.py: 300 K plus a uniform drift fast enough that, with the lists rebuilt
# every step, every atom leaves the box at least once and some atom twice in one dimension within a few dozen steps
DRIFT_CASES = {
    # (2, 2, 1) replica of the sheared 288-atom MoS2 cell, 38.3 x 44.2 x 14.0 A, xy = -19.1 A: 18 A along z, 12 A against y
    "rebomos": dict(drift=(200.0, -300.0, 450.0), nsteps=40, seed=191),
    # fcc_cell(4.045, 6), 24.27 A cubed: 29 A along x
    "aeam": dict(drift=(580.0, -200.0, 150.0), nsteps=50, seed=193),
}
_reference = {}


def drift_system(style, aeam_mass=None):
    case = DRIFT_CASES[style]
    if style == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
    else:
        s = S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)
        s.mass[1:3] = aeam_mass[:2]
    v0 = S.gaussian_velocities(s, 300.0, seed=case["seed"]) + np.array(case["drift"])
    return s, v0, case["nsteps"]


def drift_reference(oracle, style, pot_rebomos, pot_aeam):
    """the case's reference run (computed once per process): (s, v0, nsteps, {step: (x, image, xu, v)}), the lists rebuilt
    every step.  Asserts what makes the case worth running: every atom's image changes, some atom reaches |image| >= 2."""
    if style not in _reference:
        import mdref
        if style == "rebomos":
            P = oracle.rebomos_params(pot_rebomos)
            s, v0, nsteps = drift_system(style)
            make = lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)   # noqa: E731
        else:
            T = oracle.aeam_pot(pot_aeam)
            s, v0, nsteps = drift_system(style, [T.mass[0], T.mass[1]])
            make = lambda sy: mdref.AeamCPU(oracle, T, sy, skin=1.0)      # noqa: E731
        out = run(make, s, v0, nsteps, 1, {nsteps // 2, nsteps})
        image = out[nsteps][1]
        assert np.all(np.any(image != 0, axis=1)), "an atom never left the box"
        assert np.abs(image).max() >= 2, "no atom crossed the box twice in one dimension"
        _reference[style] = (s, v0, nsteps, out)
    return _reference[style]
