"""NumPy reference of the binned sums behind compute profile/mdp (csrc/profile.hip): the binning of fractional coordinates,
the terms t = (m, m vx, m vy, m vz, m v.v) of an atom, their quantised int64 sums, their exact sums (math.fsum) and the
normalisation of the compute's array.  n_edge counts the atoms a rounding of the fractional coordinate could put into the
neighbouring bin: the device forms it with fused multiply-adds, NumPy does not.  check_sums asks for none; edges and
check_sums_with_edges bracket the rows such an atom can fall in (the randomised net, which cannot choose its states)."""
import math

import numpy as np

W = 5
EDGE = 1e-9


def exponent(r, n):
    """61 - ceil(log2(max(n, 2))) - E with r < 2^E, E the frexp exponent; 0 for r == 0"""
    if not r > 0.0:
        return 0
    e = math.frexp(r)[1]
    n = max(int(n), 2)
    return 61 - (n - 1).bit_length() - e


def bins(lam, periodic, dims, nbins):
    """(row[n], n_edge): row = the bin of every atom, the first named dimension slowest; b_d = floor(s_d N_d), wrapped in a
    periodic dimension, clamped in a non-periodic one"""
    lam = np.asarray(lam, dtype=np.float64)
    row = np.zeros(len(lam), dtype=np.int64)
    edge = np.zeros(len(lam), dtype=bool)
    for d, n in zip(dims, nbins):
        u = lam[:, d] * n
        edge |= np.abs(u - np.rint(u)) < EDGE
        b = np.floor(u).astype(np.int64)
        b = ((b % n) + n) % n if periodic[d] else np.clip(b, 0, n - 1)
        row = row * n + b
    return row, int(edge.sum())


def terms(mass, v):
    mass, v = np.asarray(mass, dtype=np.float64), np.asarray(v, dtype=np.float64)
    t = np.empty((len(mass), W))
    t[:, 0] = mass
    t[:, 1:4] = mass[:, None] * v
    t[:, 4] = mass * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return t


def table(lam, periodic, dims, nbins, mass, v, exponents=None, member=None, natoms_total=None):
    """dict(count[rows] int64, sums[rows][W] int64 of rint(ldexp(t, e)), exact[rows][W] the fsum of t, absum[rows][W] the fsum
    of |t|, exponents, n_edge, rng) over the members; exponents None: from the range of the members and natoms_total"""
    rows = int(np.prod(nbins))
    row, _ = bins(lam, periodic, dims, nbins)
    t = terms(mass, v)
    keep = np.ones(len(row), dtype=bool) if member is None else np.asarray(member, dtype=bool)
    _, n_edge = bins(np.asarray(lam)[keep], periodic, dims, nbins)
    row, t = row[keep], t[keep]
    rng = np.abs(t).max(axis=0) if len(t) else np.zeros(W)
    if exponents is None:
        exponents = [exponent(r, len(lam) if natoms_total is None else natoms_total) for r in rng]
    ex = np.asarray(exponents, dtype=np.int32)
    q = np.rint(np.ldexp(t, ex)).astype(np.int64)
    count = np.bincount(row, minlength=rows).astype(np.int64)
    sums = np.zeros((rows, W), dtype=np.int64)
    np.add.at(sums, row, q)
    exact, absum = np.zeros((rows, W)), np.zeros((rows, W))
    order = np.argsort(row, kind="stable")
    cuts = np.searchsorted(row[order], np.arange(rows + 1))
    for b in np.flatnonzero(np.diff(cuts)):          # (the occupied rows: a grid may hold a million empty ones)
        tb = t[order[cuts[b]:cuts[b + 1]]]
        for k in range(W):
            exact[b, k] = math.fsum(tb[:, k])
            absum[b, k] = math.fsum(np.abs(tb[:, k]))
    return dict(count=count, sums=sums, exact=exact, absum=absum, exponents=ex, n_edge=n_edge, rng=rng)


def check_sums(count, sums, exponents, ref):
    """the device table against the reference: count exact; |sums 2^-e - fsum| <= count 2^-e + 2^-50 sum|t| for every row and
    column (half a unit per atom, doubled; the second term for the roundings of the reference's terms and the conversion).
    Returns the worst ratio to the bound."""
    assert ref["n_edge"] == 0, f"{ref['n_edge']} atoms within {EDGE} of a bin edge: the reference cannot tell their bin"
    assert np.array_equal(count, ref["count"]), np.flatnonzero(count != ref["count"])
    ex = np.asarray(exponents, dtype=np.int32)
    got = np.ldexp(np.asarray(sums, dtype=np.float64), -ex)
    bound = np.ldexp(np.asarray(count, dtype=np.float64)[:, None] * np.ones(W), -ex) + 2.0 ** -50 * ref["absum"]
    err = np.abs(got - ref["exact"])
    assert np.all(err <= bound), (err.max(), np.argwhere(err > bound)[:5])
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


def edges(lam, periodic, dims, nbins, member=None):
    """the members within EDGE of a bin edge, for check_sums_with_edges: dict(n_edge, may[rows], placed[rows]) -- may[r] the
    number of edge atoms that can fall into row r (in every dimension where the atom sits at an edge, the bin on either side
    of that edge, wrapped or clamped as bins() does), placed[r] the number of them that bins() puts there"""
    lam = np.asarray(lam, dtype=np.float64)
    rows = int(np.prod(nbins))
    keep = np.ones(len(lam), dtype=bool) if member is None else np.asarray(member, dtype=bool)
    may, placed = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    at = np.zeros(len(lam), dtype=bool)
    for d, n in zip(dims, nbins):
        u = lam[:, d] * n
        at |= np.abs(u - np.rint(u)) < EDGE
    at &= keep
    row = bins(lam, periodic, dims, nbins)[0]
    for i in np.flatnonzero(at):
        cand = [0]
        for d, n in zip(dims, nbins):
            u = float(lam[i, d]) * n
            k = int(np.rint(u))
            bs = (k - 1, k) if abs(u - k) < EDGE else (int(np.floor(u)),)
            bs = {((b % n) + n) % n if periodic[d] else min(max(b, 0), n - 1) for b in bs}
            cand = [c * n + b for c in cand for b in sorted(bs)]
        for r in set(cand):
            may[r] += 1
        assert row[i] in cand
        placed[row[i]] += 1
    return dict(n_edge=int(at.sum()), may=may, placed=placed)


def check_sums_with_edges(count, sums, exponents, ref, edge):
    """check_sums for a read that may hold atoms within EDGE of a bin edge (edge: edges() of the same read): in a row no edge
    atom can fall into, the count is exact and the sums lie within check_sums' bound; in a row one can fall into, the sums are
    skipped and the count lies between the reference's count without the edge atoms bins() put there and that plus the edge
    atoms that can fall there; the counts of all rows add to the reference's.  Returns (worst ratio to the bound, n_edge)."""
    count, rc = np.asarray(count, dtype=np.int64), np.asarray(ref["count"], dtype=np.int64)
    assert ref["n_edge"] == edge["n_edge"], (ref["n_edge"], edge["n_edge"])
    sure = edge["may"] == 0
    assert np.array_equal(count[sure], rc[sure]), np.flatnonzero(sure & (count != rc))
    low = rc - edge["placed"]
    assert np.all((count >= low) & (count <= low + edge["may"])), np.flatnonzero((count < low) | (count > low + edge["may"]))
    assert int(count.sum()) == int(rc.sum())
    ex = np.asarray(exponents, dtype=np.int32)
    got = np.ldexp(np.asarray(sums, dtype=np.float64), -ex)
    bound = np.ldexp(count.astype(np.float64)[:, None] * np.ones(W), -ex) + 2.0 ** -50 * ref["absum"]
    err = np.abs(got - ref["exact"])
    assert np.all(err[sure] <= bound[sure]), (err[sure].max(), np.argwhere((err > bound) & sure[:, None])[:5])
    ok = (bound > 0) & sure[:, None]
    return (float((err[ok] / bound[ok]).max()) if np.any(ok) else 0.0), edge["n_edge"]


def normalise(count, sums, exponents, nbins, volume, boltz, mvv2e, mv2d, com):
    """compute profile/mdp's array, one row at a time"""
    rows, ndim = int(np.prod(nbins)), len(nbins)
    out = np.zeros((rows, ndim + 7))
    vbin = volume / rows
    for b in range(rows):
        rem = b
        for k in reversed(range(ndim)):
            out[b, k] = (rem % nbins[k] + 0.5) / nbins[k]
            rem //= nbins[k]
        n = int(count[b])
        out[b, ndim] = n
        out[b, ndim + 1] = n / vbin
        if n == 0:
            continue
        t = [math.ldexp(float(int(sums[b][k])), -int(exponents[k])) for k in range(W)]
        kin = t[4] - (t[1] ** 2 + t[2] ** 2 + t[3] ** 2) / t[0] if com else t[4]
        out[b, ndim + 2] = mv2d * t[0] / vbin
        out[b, ndim + 3] = mvv2e * kin / (3.0 * n * boltz)
        out[b, ndim + 4:] = [t[1] / t[0], t[2] / t[0], t[3] / t[0]]
    return out
