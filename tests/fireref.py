"""FIRE in NumPy (tests only): the definition `minimize/mdp` and the kernels of csrc/fire.hip are held to.

This is LAMMPS `min_style fire` -- FIRE 2.0, Guenole et al., Comput. Mater. Sci. 175 (2020) 109584 -- with LAMMPS'
defaults (integrator eulerimplicit, tmax 10, tmin 0.02, delaystep 20, dtgrow 1.1, dtshrink 0.5, alpha0 0.25, alphashrink
0.99, halfstepback yes, initialdelay yes, dmax 0.1, norm two, real masses, starting time step = the current timestep),
restated from the paper and the LAMMPS documentation as its author knows them: neither the LAMMPS sources nor a
minimiser of the reference repository were at hand, so where LAMMPS does something else, this file is what the project
implements.  The points it pins down:

  * one iteration, in this order: P = sum v.f;  P > 0: s1 = 1 - alpha, s2 = alpha sqrt(sum v.v / sum f.f) (0 when
    sum f.f <= 1e-20), and if more than delaystep iterations have passed since the last P <= 0, dt = min(dt dtgrow, dtmax),
    alpha *= alphashrink;  P <= 0: remember the iteration, and -- unless initialdelay holds and fewer than delaystep
    iterations have been made -- alpha = alpha0, dt *= dtshrink if that stays >= dtmin; x -= dtv v / 2 with the dtv of the
    iteration before (halfstepback); v = 0.  Then dtv = dt, or dmax / max|v_c| if dt max|v_c| > dmax, from the velocities as
    they are NOW -- before the kick.  Then v += dtv ftm2v f / m; if P > 0: v = s1 v + s2 f; x += dtv v.
  * the limit dmax therefore bounds dtv max|v_c| of the velocities an iteration starts from; what the kick and the
    mixing add in the same iteration comes on top (small next to dmax unless the forces are huge).
  * the first iteration finds v = 0, so P = 0: it counts as a P <= 0 iteration.
  * stop tests after the forces of an iteration, in this order: etol (only when etol > 0 and more than delaystep
    iterations after the last P <= 0): |E - Eprev| < etol (|E| + |Eprev| + 1e-8) / 2;  ftol: sqrt(sum f.f) < ftol;
    maxeval: evaluations >= maxeval (the evaluation of the starting point is not counted);  then maxiter.
"""
from __future__ import annotations

import numpy as np

RUNNING, FTOL, ETOL, MAXITER, MAXEVAL = 0, 1, 2, 3, 4
CRITERION = {FTOL: "force tolerance", ETOL: "energy tolerance", MAXITER: "max iterations", MAXEVAL: "max force evaluations"}
DEFAULTS = dict(dmax=0.1, tmax=10.0, tmin=0.02, delaystep=20, dtgrow=1.1, dtshrink=0.5, alpha0=0.25, alphashrink=0.99,
                halfstepback=True, initialdelay=True)


class Fire:
    """state of a minimisation; m: masses per atom [n]; dt: the starting time step"""

    def __init__(self, x, m, dt, ftm2v, v=None, **modify):
        unknown = set(modify) - set(DEFAULTS)
        assert not unknown, unknown
        self.__dict__.update(DEFAULTS)
        self.__dict__.update(modify)
        self.x = np.array(x, dtype=np.float64)
        self.v = np.zeros_like(self.x) if v is None else np.array(v, dtype=np.float64)
        self.m = np.asarray(m, dtype=np.float64)[:, None]
        self.ftm2v = ftm2v
        self.dt, self.dtmax, self.dtmin = dt, self.tmax * dt, self.tmin * dt
        self.alpha = self.alpha0
        self.dtv = dt                 # of the last iteration (halfstepback)
        self.iter = self.last_negative = self.negatives = self.evaluations = 0
        self.s1, self.s2, self.mixed, self.vdotf = 1.0, 0.0, False, 0.0

    def advance(self, f):
        """steps 1-4 of one iteration with the forces f at the current positions"""
        f = np.asarray(f, dtype=np.float64)
        x, v = self.x, self.v
        self.iter += 1
        self.vdotf = float((v * f).sum())
        self.mixed = self.vdotf > 0.0
        if self.mixed:
            vv, ff = float((v * v).sum()), float((f * f).sum())
            self.s1 = 1.0 - self.alpha
            self.s2 = 0.0 if ff <= 1e-20 else self.alpha * np.sqrt(vv / ff)
            if self.iter - self.last_negative > self.delaystep:
                self.dt = min(self.dt * self.dtgrow, self.dtmax)
                self.alpha *= self.alphashrink
        else:
            self.s1, self.s2 = 1.0, 0.0
            self.last_negative = self.iter
            self.negatives += 1
            if not (self.initialdelay and self.iter < self.delaystep):
                self.alpha = self.alpha0
                if self.dt * self.dtshrink >= self.dtmin:
                    self.dt *= self.dtshrink
            if self.halfstepback:
                x -= 0.5 * self.dtv * v
            v[:] = 0.0
        vmax = float(np.abs(v).max()) if v.size else 0.0
        self.dtv = self.dt if self.dt * vmax <= self.dmax else self.dmax / vmax
        v += self.dtv * self.ftm2v * f / self.m
        if self.mixed:
            v[:] = self.s1 * v + self.s2 * f
        x += self.dtv * v

    def stop_test(self, f, e, e_prev, etol, ftol, maxiter, maxeval):
        """step 5, with the forces (and energies, when etol > 0) of the iteration just advanced"""
        self.evaluations += 1
        if etol > 0.0 and self.iter - self.last_negative > self.delaystep and \
                abs(e - e_prev) < etol * 0.5 * (abs(e) + abs(e_prev) + 1e-8):
            return ETOL
        if np.sqrt(float((np.asarray(f) ** 2).sum())) < ftol:
            return FTOL
        if self.evaluations >= maxeval:
            return MAXEVAL
        if self.iter >= maxiter:
            return MAXITER
        return RUNNING


def minimize(force_energy, x, m, dt, ftm2v, etol, ftol, maxiter, maxeval, record=None, **modify):
    """force_energy(x) -> (f, e).  Returns dict(x, v, f, stop, iterations, evaluations, e_initial, e_previous, e_final,
    fnorm_initial, fnorm, dt, alpha, negatives: the iterations with P <= 0).  record(fire, f): called after every
    iteration's forces."""
    s = Fire(x, m, dt, ftm2v, **modify)
    f, e = force_energy(s.x)
    e0 = e_prev = e
    fn0 = float(np.sqrt((f * f).sum()))
    negatives = []
    stop = MAXITER if maxiter <= 0 else RUNNING
    while stop == RUNNING:
        s.advance(f)
        if not s.mixed:
            negatives.append(s.iter)
        e_prev = e
        f, e = force_energy(s.x)
        if record is not None:
            record(s, f)
        stop = s.stop_test(f, e, e_prev, etol, ftol, maxiter, maxeval)
    return dict(x=s.x, v=s.v, f=f, stop=stop, iterations=s.iter, evaluations=s.evaluations, e_initial=e0, e_previous=e_prev,
                e_final=e, fnorm_initial=fn0, fnorm=float(np.sqrt((f * f).sum())), dt=s.dt, alpha=s.alpha,
                negatives=negatives, state=s)
