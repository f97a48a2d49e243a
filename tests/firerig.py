"""What the FIRE tests share (tests/test_gpu_fire_mdp.py, the `fire` net of tests/nets.py and its corner test in
tests/test_net_draws.py): the start cells, the oracle engine that keeps its lists valid while atoms move, the rig (a
context with one resident brick) and the REPLAY -- every iteration of the device repeated by ONE fireref iteration from
the device's own downloaded state and forces.  A helper module, not a test module."""
from __future__ import annotations

import numpy as np

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
import fireref
import mdref
from refloops import worse

DT = 0.001
BIG = 10 ** 9
SKIN = {"rebomos": 2.0, "aeam": 1.0}


def cell(style, hot=False, jitter=None, scale=1.0, seed=None):
    """the start cells of the FIRE tests.  hot: the large strained ones.  jitter / scale / seed: the small cell of the
    style with another jitter amplitude (A), strain and jitter seed (the `fire` net)"""
    if style == "rebomos":
        if hot:
            return S.jitter(S.scale(S.replicate(S.rebomos_bulk_cell(), (2, 2, 2)), 1.12), 0.3, 31)
        s = S.rebomos_bulk_cell()
        if scale != 1.0:
            s = S.scale(s, scale)
        return S.jitter(s, 0.05 if jitter is None else jitter, seed=11 if seed is None else seed)
    af = capi.AeamFile(POT_AEAM)
    s = S.fcc_cell(4.045, 10, frac_type2=0.08, seed=51) if hot else S.fcc_cell(4.045, 4, frac_type2=0.08, seed=5)
    s.mass[1:3] = af.mass[:2]
    if hot:
        return S.jitter(s, 0.3, 32)
    if scale != 1.0:
        s = S.scale(s, scale)
    return S.jitter(s, 0.05 if jitter is None else jitter, seed=21 if seed is None else seed)


class Forces:
    """the oracle's forces (and energy) at any positions of the system `s`: the lists are built anew whenever an atom
    has moved a quarter of the skin since the last build, so they are valid by construction (a list built with a skin
    holds while no atom has moved half of it)"""

    def __init__(self, style, oracle, s, skin=None):
        self.style, self.orc, self.s = style, oracle, s
        self.skin = SKIN[style] if skin is None else skin
        self.pot = oracle.rebomos_params(POT_REBOMOS) if style == "rebomos" else oracle.aeam_pot(POT_AEAM)
        self.eng, self.x0, self.builds = None, None, 0

    def _dx(self, dx):
        return dx - np.round(self.s.box.x2lamda(dx + self.s.box.lo)) @ self.s.box.h.T

    def __call__(self, x, eflag=0):
        d = None if self.eng is None else self._dx(x - self.x0)    # (x may have been wrapped since: the same atom, another image)
        if d is None or np.sqrt((d ** 2).sum(axis=1)).max() > 0.25 * self.skin:
            self.x0 = S.wrap(self.s.box, x)
            sy = S.System(self.s.box, self.x0.copy(), self.s.type, self.s.tag, self.s.mass)
            cls = mdref.RebomosCPU if self.style == "rebomos" else mdref.AeamCPU
            self.eng, self.builds, d = cls(self.orc, self.pot, sy, skin=self.skin), self.builds + 1, 0.0
        return self.eng.compute(self.x0 + d, eflag=eflag, vflag=0)


class Rig:
    """a context with one resident brick of `s`, and the oracle engine for the same potential"""

    def __init__(self, style, s, oracle, v0=None, dt=DT):
        self.style, self.s, self.orc, self.dt = style, s, oracle, dt
        self.ctx = capi.Context(0)
        self.skin = SKIN[style]
        if style == "rebomos":
            p = capi.read_rebomos_file(POT_REBOMOS)
            self.ctx.rebomos_set_params(p)
            self.P = oracle.rebomos_params(POT_REBOMOS)
            self.d = resident.DeviceDomain(self.ctx, capi.STYLE_REBOMOS, s, 3.0 * p.rcmax[0][0] + self.skin, self.skin, [0, 0, 1],
                                           v0=v0, dt=dt)
        else:
            af = capi.AeamFile(POT_AEAM)
            tabs = af.build()
            self.ctx.aeam_set_tables(tabs)
            self.T = oracle.aeam_pot(POT_AEAM)
            self.d = resident.DeviceDomain(self.ctx, capi.STYLE_AEAM, s, float(af.cut_table(tabs).max()) + self.skin, self.skin,
                                           None, v0=v0, dt=dt)
        self.m = s.mass[s.type]

    def engine(self, x):
        sy = S.System(self.s.box, np.ascontiguousarray(x), self.s.type, self.s.tag, self.s.mass)
        if self.style == "rebomos":
            return mdref.RebomosCPU(self.orc, self.P, sy, skin=self.skin)
        return mdref.AeamCPU(self.orc, self.T, sy, skin=self.skin)

    def by_tag(self, want=("x", "v", "f")):
        got = self.ctx.md_download(self.d.nlocal, want=want)
        idx = self.ctx.md_download_int("tag", self.d.nlocal) - 1
        out = {}
        for k in want:
            a = np.zeros((self.s.n, 3))
            a[idx] = got[k]
            out[k] = a
        return out

    def unwrap(self, dx):
        return dx - np.round(self.s.box.x2lamda(dx + self.s.box.lo)) @ self.s.box.h.T

    def close(self):
        self.ctx.close()


def replay(rig, niter, modify=None, forces=False):
    """niter device iterations, one at a time, each against one fireref iteration (with the min_modify settings `modify`
    and the rig's starting time step) from the device's own state.  An iteration with |cos(v, f)| < 1e-9 is not replayed:
    its branch hangs on the order of the sums.  forces: the downloaded forces of every iteration also against the
    oracle's at the downloaded positions.  Nothing is asserted here; returns
      exact     what was decided, not summed (branch, counters, dt, alpha), and differs: [(iteration, text)]
      x, v, ctl the worst deviations: positions (A), velocities (relative per atom), dtv / s1 / s2 (relative)
      f         the worst |f - f_oracle| (eV/A; 0.0 without `forces`)
      negatives the iterations with P <= 0;  grown, limited, skipped, ceiling: iterations whose dt grew, whose dtv dmax
                shortened, that were not replayed, that ended with dt == dtmax;  moved: the farthest an atom went (A)"""
    ctx, modify = rig.ctx, dict(modify or {})
    orc_f = Forces(rig.style, rig.orc, rig.s, rig.skin) if forces else None
    st = ctx.fire_state()
    a = rig.by_tag()
    x_start = a["x"]
    out = dict(exact=[], x=0.0, v=0.0, ctl=0.0, f=0.0, negatives=[], grown=0, limited=0, skipped=0, ceiling=0, moved=0.0)
    dtmax = modify.get("tmax", fireref.DEFAULTS["tmax"]) * rig.dt
    for it in range(1, niter + 1):
        stop = ctx.fire_iterate(1)
        if stop:
            out["exact"].append((it, f"fire_iterate returned the stop code {stop}"))
            break
        st2 = ctx.fire_state()
        b = rig.by_tag()
        vn, fn = np.sqrt((a["v"] ** 2).sum()), np.sqrt((a["f"] ** 2).sum())
        cos = abs((a["v"] * a["f"]).sum()) / (vn * fn) if vn > 0.0 else 1.0
        if not st2["mixed"]:
            out["negatives"].append(it)
        if cos < 1e-9:                  # the branch hangs on the order of the sums
            out["skipped"] += 1
        else:
            r = fireref.Fire(a["x"], rig.m, rig.dt, S.FTM2V, v=a["v"], **modify)
            r.dt, r.alpha, r.dtv = st["dt"], st["alpha"], st["dtv"]
            r.iter, r.last_negative, r.negatives = st["iterations"], st["last_negative"], st["negatives"]
            r.advance(a["f"])
            # the branch and everything that is decided, not summed: exactly
            ref = (r.mixed, r.iter, r.last_negative, r.negatives, not r.mixed, r.dt, r.alpha)
            dev = (bool(st2["mixed"]), st2["iterations"], st2["last_negative"], st2["negatives"], bool(st2["zeroed"]), st2["dt"],
                   st2["alpha"])
            if ref != dev:
                out["exact"].append((it, f"(mixed, iter, last_negative, negatives, zeroed, dt, alpha) {dev}, reference {ref}"))
            for k, want in (("dtv", r.dtv), ("s1", r.s1), ("s2", r.s2)):
                out["ctl"] = worse(out["ctl"], abs(st2[k] - want) / abs(want) if want != 0.0 else abs(st2[k]))
            out["x"] = worse(out["x"], float(np.abs(rig.unwrap(b["x"] - r.x)).max()))
            out["v"] = worse(out["v"], float((np.sqrt(((b["v"] - r.v) ** 2).sum(axis=1)) / np.sqrt((r.v ** 2).sum(axis=1))).max()))
            out["grown"] += st2["dt"] > st["dt"]
            out["limited"] += st2["dtv"] < st2["dt"]
            out["ceiling"] += st2["dt"] == dtmax
        if forces:
            out["f"] = worse(out["f"], float(np.abs(orc_f(b["x"])["f_owned"] - b["f"]).max()))
        out["moved"] = max(out["moved"], float(np.sqrt((rig.unwrap(b["x"] - x_start) ** 2).sum(axis=1)).max()))
        st, a = st2, b
    return out
