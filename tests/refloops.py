"""What the reference side of several test modules shares (tests/test_gpu_langevin_mdp.py, tests/nets.py,
tests/firerig.py): the host loop of the Langevin tests -- velocity Verlet + tests/langevinref.py around the oracle -- and
the NaN-keeping maximum of the report values.  A helper module, not a test module; no GPU."""
from __future__ import annotations

import numpy as np

from lammps_plugins_amd.host import system as S


def worse(a, b):
    """the larger of two deviations; a NaN stays (max() would drop it, and a NaN must fail a bound)"""
    return a if a != a or b <= a else b


def host_lgv(make_engine, s, v0, nsteps, every, rebuild_every, lgv, dt=0.001, first=0, last=None, skin=None):
    """velocity Verlet + Langevin around the oracle, the run's steps numbered first + 1 .. first + nsteps with the ramp
    ending at `last` (default: the run's last step; steps beyond it hold Tstop), in the box of `s` (sheared or not);
    {step of the run, 1 .. nsteps: (x by tag, thermostat energy, v by tag)}.  The lists are built anew every
    rebuild_every steps; skin: assert that no atom has moved more than half of it since the last build -- the reference
    itself then cannot have missed a pair."""
    m = s.mass[s.type][:, None]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    x_built = x.copy()
    lgv.setup(first, first + nsteps if last is None else last)
    f = eng.compute(x, eflag=1, vflag=0)["f_owned"] + lgv.force(first, s.tag, s.type, v, phase=1)
    lgv.tally_setup(v)
    dtf = 0.5 * dt * S.FTM2V
    out = {}
    for step in range(1, nsteps + 1):
        v += dtf * f / m
        x += dt * v
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
            x_built = x.copy()
        elif skin is not None:
            far = float(np.sqrt(((x - x_built) ** 2).sum(axis=1)).max())
            assert far <= 0.5 * skin, f"the reference's own list is stale at step {step}: an atom moved {far:.3f} A"
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"] + lgv.force(first + step, s.tag, s.type, v)
        v += dtf * f / m
        lgv.tally_step(v)
        if step in every:
            out[step] = (x.copy(), lgv.scalar(), v.copy())
    return out
