"""NumPy reference of the binned sums behind compute profile/mdp (csrc/profile.hip): the binning of fractional coordinates,
the terms t = (m, m vx, m vy, m vz, m v.v) of an atom, their quantised int64 sums, their exact sums (math.fsum) and the
normalisation of the compute's array.  n_edge counts the atoms a rounding of the fractional coordinate could put into the
neighbouring bin: the device forms it with fused multiply-adds, NumPy does not."""
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
    for b in range(rows):
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
