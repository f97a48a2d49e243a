"""NumPy reference of compute coord/atom/mdp and centro/atom/mdp (LAMMPS compute coord/atom cutoff, compute centro/atom
without axes) for their tests: a brute force over every atom pair and every periodic image, on rdfref._pairs_in_range and
adfref.neighbours.

x[n][3] and types[n] are by tag (row t - 1 = the atom with tag t), h the 3 x 3 box matrix whose COLUMNS are the box vectors
(system.Box.h), periodic three flags, member[n] booleans by tag or None: the CENTRES.  A partner is any other entry (atom,
image) of any group, the centre's own images included, with rsq < cutoff^2 (include/mdpair_hip.h, mdp_coord_read).

coord: a device that forms the same rsq up to its last bit counts a pair differently only if rsq is within rounding of
cutoff^2.  So a pair with rsq < cutoff^2 (1 - EDGE) is SURE and one with |rsq / cutoff^2 - 1| < EDGE is an EDGE pair (EDGE =
rdfref.EDGE = 1e-9, relative); a device count is right when count_sure <= device <= count_sure + edge.

centro: only the choice of the N nearest is discontinuous in the positions -- the sum of the N / 2 smallest pair values is
continuous in them (the k-th smallest of a set of continuous functions is continuous) -- so an atom is AMBIGUOUS where the
N-th and the (N + 1)-th rsq inside the cutoff differ by less than AMBIGUOUS = 1e-9 relative, or where the N-th lies within
that of cutoff^2, and the tests compare every other atom."""
import numpy as np

import adfref
import rdfref

EDGE = rdfref.EDGE
AMBIGUOUS = 1e-9


def coord(x, types, h, periodic, cutoff, ranges, member=None):
    """ranges: [(jlo, jhi), ...] inclusive type ranges, one column each.  dict(count_sure[n][ncol], edge[n][ncol], n_edge)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    types = np.asarray(types)
    h = np.asarray(h, dtype=np.float64)
    n, ncol = len(x), len(ranges)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member).astype(bool)
    in_j = np.array([(types >= lo) & (types <= hi) for lo, hi in ranges])
    sure = np.zeros((n, ncol), dtype=np.int64)
    edge = np.zeros((n, ncol), dtype=np.int64)
    n_edge = 0
    for i, j, r in rdfref._pairs_in_range(x, h, periodic, cutoff * (1.0 + 1e-6)):
        t = r * r / (cutoff * cutoff)
        is_edge = np.abs(t - 1.0) < EDGE
        is_sure = (t < 1.0) & ~is_edge
        keep = member[i]
        n_edge += int((is_edge & keep).sum())
        for m in range(ncol):
            sel = keep & in_j[m, j]
            sure[:, m] += np.bincount(i[sel & is_sure], minlength=n)
            edge[:, m] += np.bincount(i[sel & is_edge], minlength=n)
    return dict(count_sure=sure, edge=edge, n_edge=n_edge)


def centro_of(d, nnn):
    """the parameter of one centre from the displacements d[k][3] of ALL its partners inside the cutoff (k >= nnn): the nnn nearest,
    their nnn (nnn - 1) / 2 values |R_a + R_b|^2, the nnn / 2 smallest added in ascending order"""
    rsq = (d * d).sum(axis=1)
    near = d[np.argsort(rsq, kind="stable")[:nnn]]
    a, b = np.triu_indices(nnn, 1)
    u = near[a] + near[b]
    pv = np.sort(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
    s = 0.0
    for v in pv[:nnn // 2]:
        s += float(v)
    return s


def centro(x, h, periodic, nnn, cutoff, member=None):
    """dict(value[n], inside[n], ambiguous[n]): the parameter per atom (0 outside the group and with fewer than nnn inside the
    cutoff), the number of partners inside the cutoff, and the flag of the module docstring"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = len(x)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member).astype(bool)
    i, j, d, rsq = adfref.neighbours(x, h, periodic, cutoff)
    order = np.argsort(i, kind="stable")
    i, d, rsq = i[order], d[order], rsq[order]
    start = np.searchsorted(i, np.arange(n + 1))
    value, inside, amb = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for k in range(n):
        lo, hi = start[k], start[k + 1]
        inside[k] = hi - lo
        if not member[k]:
            continue
        r = np.sort(rsq[lo:hi])
        # a partner within rounding of the cutoff may or may not be there for the device
        near_cut = bool(np.any(np.abs(r / (cutoff * cutoff) - 1.0) < AMBIGUOUS))
        if hi - lo < nnn:
            amb[k] = near_cut
            continue
        if hi - lo > nnn and r[nnn] - r[nnn - 1] < AMBIGUOUS * r[nnn]:
            amb[k] = True
        if near_cut and hi - lo == nnn:
            amb[k] = True
        value[k] = centro_of(d[lo:hi], nnn)
    return dict(value=value, inside=inside, ambiguous=amb)


def centro_bound(nnn, cutoff, lmax):
    """|device - reference| for an unambiguous atom: the roundings of x + shift and of the differences, about 4 eps lmax per
    component, carried through 2 (2 cutoff) per square, three components and nnn / 2 terms, with a margin of about 3:
    64 eps nnn cutoff lmax"""
    return 64.0 * np.finfo(np.float64).eps * nnn * cutoff * lmax
