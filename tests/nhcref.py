"""NumPy restatement of the Nose-Hoover chain thermostat of LAMMPS fix nvt (FixNH: Martyna-Tuckerman-Klein chain,
thermostat only) as the device implements it (csrc/nhc.hip, include/mdpair_hip.h "Nose-Hoover chain"): the host
reference of the `fix nvt/mdp` tests.

Use around velocity Verlet, one step n of a run from `first` to `last`:
    initial:  nhc.begin_step(n);  v *= nhc.half();  v += dtf f/m;  x += dt v
    final:    v += dtf f/m;  v *= nhc.half(nhc.temperature(v, m))
with nhc.setup(v, m, first, last) at the start of every run."""
from __future__ import annotations

import math

import numpy as np


class NHC:
    def __init__(self, t_start, t_stop, t_period, nf, dt, tchain=3, tloop=1, drag=0.0, boltz=8.617343e-5,
                 mvv2e=1.0364269e-4):
        assert t_start > 0 and t_stop > 0 and t_period > 0 and tchain >= 1 and tloop >= 1
        self.t_start, self.t_stop, self.t_freq = t_start, t_stop, 1.0 / t_period
        self.nf, self.dt, self.M, self.L, self.drag = float(nf), dt, tchain, tloop, drag
        self.kb, self.mvv2e = boltz, mvv2e
        self.eta = [0.0] * tchain
        self.eta_dot = [0.0] * (tchain + 1)      # eta_dot[M] == 0
        self.eta_dotdot = [0.0] * tchain
        self.Q = [0.0] * tchain
        self.first = self.last = 0
        self.tt = t_start
        self.T = 0.0

    # ---- pieces
    def temperature(self, v, m):
        ke = 0.5 * self.mvv2e * float(np.sum(m * np.sum(v * v, axis=1)))
        return 2.0 * ke / (self.nf * self.kb) if self.nf > 0 else 0.0

    def target(self, n):
        delta = 0.0 if self.last == self.first else (n - self.first) / (self.last - self.first)
        return self.t_start + delta * (self.t_stop - self.t_start)

    def _masses(self, tt):
        kt, tf2 = self.kb * tt, self.t_freq ** 2
        self.Q[0] = self.nf * kt / tf2
        for i in range(1, self.M):
            self.Q[i] = kt / tf2

    # ---- the fix
    def setup(self, v, m, first, last):
        """FixNH::setup of a run from step first to step last"""
        self.first, self.last = first, last
        self.tt = self.target(first)
        self.T = self.temperature(v, m)
        self._masses(self.tt)
        for i in range(1, self.M):
            self.eta_dotdot[i] = (self.Q[i - 1] * self.eta_dot[i - 1] ** 2 - self.kb * self.tt) / self.Q[i]

    def begin_step(self, n):
        self.tt = self.target(n)

    def half(self, T=None):
        """one half-update at the current target; T: the temperature now (None: carried from the last update).
        Returns the velocity scale factor."""
        if T is not None:
            self.T = T
        M, L, dt = self.M, self.L, self.dt
        ed, edd, Q, eta = self.eta_dot, self.eta_dotdot, self.Q, self.eta
        kt = self.kb * self.tt
        ket = self.nf * kt
        self._masses(self.tt)
        edd[0] = (self.nf * self.kb * self.T - ket) / Q[0] if Q[0] > 0 else 0.0
        w = 1.0 / L
        tdrag = 1.0 - dt * self.t_freq * self.drag / L
        S = 1.0
        for _ in range(L):
            for i in range(M - 1, 0, -1):
                a = math.exp(-w * dt / 8 * ed[i + 1])
                ed[i] = ((ed[i] * a + edd[i] * w * dt / 4) * tdrag) * a
            a = math.exp(-w * dt / 8 * ed[1])
            ed[0] = ((ed[0] * a + edd[0] * w * dt / 4) * tdrag) * a
            s = math.exp(-w * dt / 2 * ed[0])
            S *= s
            self.T *= s * s
            edd[0] = (self.nf * self.kb * self.T - ket) / Q[0] if Q[0] > 0 else 0.0
            for i in range(M):
                eta[i] += w * dt / 2 * ed[i]
            ed[0] = (ed[0] * a + edd[0] * w * dt / 4) * a
            for i in range(1, M):
                a = math.exp(-w * dt / 8 * ed[i + 1])
                ed[i] *= a
                edd[i] = (Q[i - 1] * ed[i - 1] ** 2 - kt) / Q[i]
                ed[i] += edd[i] * w * dt / 4
                ed[i] *= a
        return S

    def energy(self):
        """compute_scalar (ecouple) at the current target"""
        kt = self.kb * self.tt
        e = self.nf * kt * self.eta[0] + 0.5 * self.Q[0] * self.eta_dot[0] ** 2
        for i in range(1, self.M):
            e += kt * self.eta[i] + 0.5 * self.Q[i] * self.eta_dot[i] ** 2
        return e


def run_nvt(x, v, m, force, nhc: NHC, first, last, ftm2v, on_step=None):
    """velocity Verlet + chain from step first to last; force(x) -> (f, pe).  on_step(n, x, v, pe) after each step."""
    dt = nhc.dt
    f, pe = force(x)
    nhc.setup(v, m, first, last)
    dtf = 0.5 * dt * ftm2v
    for n in range(first + 1, last + 1):
        nhc.begin_step(n)
        v *= nhc.half()
        v += dtf * f / m[:, None]
        x += dt * v
        f, pe = force(x)
        v += dtf * f / m[:, None]
        v *= nhc.half(nhc.temperature(v, m))
        if on_step is not None:
            on_step(n, x, v, pe)
    return x, v
