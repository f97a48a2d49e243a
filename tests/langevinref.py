"""NumPy restatement of the Langevin thermostat of LAMMPS fix langevin (FixLangevin::post_force without gjf / angmom /
omega, with zero and tally) as the device implements it (csrc/langevin.hip, include/mdpair_hip.h "Langevin"): the host
reference of the `fix langevin/mdp` tests.  The noise is Philox4x32-10 keyed by (seed, tag, step, phase), not LAMMPS'
per-rank Marsaglia stream.

Use around velocity Verlet, a run from step `first` to `last`:
    lgv.setup(first, last);  f += lgv.force(first, tag, type, v, phase=1);  lgv.tally_setup(v)
    per step n:  v += dtf f/m;  x += dt v;  f = pair(x);  fl = lgv.force(n, tag, type, v);  f += fl
                 v += dtf f/m;  lgv.tally_step(v)
and lgv.scalar() is compute_scalar()."""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: [4, n] (or [4]) unsigned 32-bit words, key: (k0, k1); returns the four output words, uint32, same shape"""
    c = [np.asarray(w, dtype=np.uint64) & MASK for w in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]          # 64-bit products of 32-bit words
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    return [w.astype(np.uint32) for w in c]


def uniform(r):
    """a 32-bit word -> u in (0, 1): (r + 0.5) 2^-32"""
    return (np.asarray(r, dtype=np.float64) + 0.5) * 2.0 ** -32


def noise(seed, tag, step, phase):
    """[n, 3] uniforms of the atoms `tag` at `step` (phase 0: post_force, 1: the setup force)"""
    tag = np.asarray(tag, dtype=np.uint64)
    n = tag.shape[0]
    st = int(step)
    ctr = [tag, np.full(n, st & 0xFFFFFFFF, np.uint64), np.full(n, (st >> 32) & 0xFFFFFFFF, np.uint64),
           np.full(n, phase, np.uint64)]
    w = philox4x32_10(ctr, (seed, 0))
    return np.stack([uniform(w[0]), uniform(w[1]), uniform(w[2])], axis=1)


class Langevin:
    def __init__(self, t_start, t_stop, damp, seed, mass, dt, ftm2v, boltz=8.617343e-5, mvv2e=1.0364269e-4,
                 ratio=None, zero=False, tally=False):
        """mass: [ntypes + 1] per type (index 0 unused); ratio: {type: ratio} of `scale`"""
        assert damp > 0 and seed > 0 and t_start >= 0 and t_stop >= 0
        self.t_start, self.t_stop, self.seed, self.dt = t_start, t_stop, seed, dt
        self.zero, self.tally = zero, tally
        mass = np.asarray(mass, dtype=np.float64)
        r = np.ones(len(mass))
        for t, v in (ratio or {}).items():
            r[t] = v
        self.g1 = -mass / damp / ftm2v
        self.g2 = np.sqrt(mass) * np.sqrt(24.0 * boltz / damp / dt / mvv2e) / ftm2v
        self.g1 *= 1.0 / r
        self.g2 *= 1.0 / np.sqrt(r)
        self.first = self.last = 0
        self.energy = self.e_last = 0.0
        self.fl = None

    def setup(self, first, last):
        self.first, self.last = first, last

    def target(self, n):
        delta = 0.0 if self.last == self.first else (n - self.first) / (self.last - self.first)
        delta = min(max(delta, 0.0), 1.0)
        return self.t_start + delta * (self.t_stop - self.t_start)

    def random(self, n, tag, type_, phase=0):
        """fran: gamma2 (u - 0.5), [natoms, 3]"""
        g2 = self.g2[type_] * np.sqrt(self.target(n))
        return g2[:, None] * (noise(self.seed, tag, n, phase) - 0.5)

    def force(self, n, tag, type_, v, phase=0):
        """f_L of step n (phase 1: the setup force of the run) for velocities v; kept for the tally"""
        fran = self.random(n, tag, type_, phase)
        fl = self.g1[type_][:, None] * v + fran
        if self.zero:
            fl -= fran.sum(axis=0) / len(tag)
        self.fl = fl
        return fl

    def tally_setup(self, v):
        """compute_scalar at the run's first step: energy = 0.5 E_setup dt"""
        self.e_last = float(np.sum(self.fl * v))
        self.energy = 0.5 * self.e_last * self.dt

    def tally_step(self, v):
        """end_of_step: v after the final half"""
        self.e_last = float(np.sum(self.fl * v))
        self.energy += self.e_last * self.dt

    def scalar(self):
        return -(self.energy - 0.5 * self.e_last * self.dt) if self.tally else 0.0


def run_langevin(x, v, mass_atom, tag, type_, force, lgv: Langevin, first, last, ftm2v, on_step=None):
    """velocity Verlet + Langevin from step first to last; force(x) -> (f, pe).  on_step(n, x, v, pe) after each step."""
    dt = lgv.dt
    dtf = 0.5 * dt * ftm2v
    m = mass_atom[:, None]
    lgv.setup(first, last)
    f, pe = force(x)
    f = f + lgv.force(first, tag, type_, v, phase=1)
    lgv.tally_setup(v)
    for n in range(first + 1, last + 1):
        v += dtf * f / m
        x += dt * v
        f, pe = force(x)
        f = f + lgv.force(n, tag, type_, v)
        v += dtf * f / m
        lgv.tally_step(v)
        if on_step is not None:
            on_step(n, x, v, pe)
    return x, v
