"""CPU check of the candidate-row order (cand_order_kernel, csrc/rebomos.hip): which trips d of the centre kernels' first
pair loop hold a pair (m, m + d mod n) with cos >= 1/2, for every Mo centre with 12 neighbours of the benchmark's cell
replicated 4 x 4 x 2 (3072 Mo centres), brute force, rcmax from the potential file.

  python profiles/slot_order/trip_sets.py            # lattice and Gaussian jitter sigma = 0.08 A

Orders compared: the sweep order of the bin grid (z, then y, then x) and the azimuth order of the kernel (lab axis of the
smallest sum of d^2, atan2 in the plane of the other two, ties by the coordinate along the axis, then by the old place)."""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from lammps_plugins_amd.host import capi, system as S  # noqa: E402


def neighbours(s, rc):
    """per owned Mo atom: the d vectors of the atoms within rc[Mo][tj], periodic images included"""
    xa, type_all, _, _, _, _, _ = S.with_ghosts(s, float(np.max(rc)) + 0.5)
    rc2 = rc[0][type_all - 1] ** 2
    out = []
    for i in np.flatnonzero(s.type == 1):
        d = xa - xa[i]
        r2 = (d ** 2).sum(axis=1)
        out.append(d[(r2 < rc2) & (r2 > 0.0)])
    return out


def azimuth_order(d):
    sxx, syy, szz = (d ** 2).sum(axis=0)
    axis = 2 if (szz <= sxx and szz <= syy) else (1 if syy <= sxx else 0)
    a, b = {2: (0, 1), 1: (2, 0), 0: (1, 2)}[axis]
    az = np.arctan2(d[:, b], d[:, a])
    return np.lexsort((np.arange(len(d)), d[:, axis], az))


def sweep_order(d):
    return np.lexsort((d[:, 0], d[:, 1], d[:, 2]))


def trips(d):
    n = len(d)
    u = d / np.linalg.norm(d, axis=1)[:, None]
    cs = u @ u.T
    hit = set()
    for k in range(1, n // 2 + 1):
        ms = range(n) if 2 * k < n else range(k)
        if any(cs[m, (m + k) % n] >= 0.5 for m in ms):
            hit.add(k)
    return tuple(sorted(hit))


def main():
    p = capi.read_rebomos_file(os.path.join(ROOT, "tests", "golden", "potentials", "MoS.REBO.set5b"))
    rc = np.array([[p.rcmax[a][b] for b in range(2)] for a in range(2)])
    base = S.replicate(S.rebomos_bulk_cell(), (4, 4, 2))
    rng = np.random.default_rng(8)
    for name, s in (("lattice", base),
                    ("Gaussian jitter 0.08 A", S.System(base.box, S.wrap(base.box, base.x + rng.normal(0.0, 0.08, base.x.shape)),
                                                         base.type, base.tag, base.mass))):
        nb = neighbours(s, rc)
        for oname, order in (("sweep order", sweep_order), ("azimuth order", azimuth_order)):
            sets = Counter()
            for d in nb:
                if len(d) == 12:
                    sets[trips(d[order(d)])] += 1
            print(f"{name}, {oname}: " + ", ".join(f"{n} centres {set(k) if k else '{}'}" for k, n in sorted(sets.items())))


if __name__ == "__main__":
    main()
