"""NumPy reference of compute adf/mdp (LAMMPS compute adf) for its tests: a brute force over every centre, every neighbour
in every periodic image and every ordered pair of neighbours, in integers, with the compute's normalisation on top.

counts(x, types, h, periodic, nbin, ordinate, triples, member): x[n][3] and types[n] by tag (row t - 1 = the atom with tag
t), h the 3 x 3 box matrix whose COLUMNS are the box vectors (system.Box.h), periodic three flags, ordinate "degree",
"radian" or "cosine", triples a list of (ilo, ihi, jlo, jhi, klo, khi, rjin, rjout, rkin, rkout) with inclusive type
ranges, member[n] booleans by tag or None.  The semantics are those of include/mdpair_hip.h (mdp_adf_counts): a centre is
a member with its type in the i range; a neighbour is any other entry (atom, image), the centre's own images included; it
is a j-neighbour when it is a member, its type fits and rjin^2 <= rsq < rjout^2, a k-neighbour by the same rule; every
ordered pair (j, k) of different entries counts once at b = (int) ((u - lo) nbin / (hi - lo)), b >= nbin going into the
last bin.  Image positions are formed as x + shift and the difference taken from that, as the device's ghosts are.

A device that forms the same cosine up to its last bits puts an angle into another bin only if (u - lo) nbin / (hi - lo)
is within rounding of an integer strictly between 0 and nbin (bin 0 and bin nbin - 1 have no outer edge, so the window
does not shrink where acos is steep).  Every angle is SURE (at least EDGE = 1e-9 of a bin away from such an integer) or
EDGE; a device histogram is right when hist_sure <= device <= hist_sure + edge_adjacent in every counter.  Two algebraically
equal forms of the cosine differ by at most 2e-12 of a bin at interior edges (jittered fcc, nbin up to 180, all three
ordinates), so 1e-9 leaves three decades.  n_shell_edge counts the member neighbours of centres whose rsq lies within a relative 1e-9 of a
squared shell radius: there the last bit would decide membership of a shell, not merely a bin, and check_bracket refuses
such an input."""
import math

import numpy as np

from rdfref import _shift_ranges

EDGE = 1e-9
RANGE = dict(degree=(0.0, 180.0), radian=(0.0, math.pi), cosine=(-1.0, 1.0))


def neighbours(x, h, periodic, rmax):
    """(i, j, d[.][3], rsq) of every ordered pair (i, j + image) with rsq < rmax^2, (j, image) != (i, 0), sorted by i"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    nsh = _shift_ranges(x, h, periodic, rmax)
    lo, hi = x.min(axis=0), x.max(axis=0)
    out = []
    for kx in range(-nsh[0], nsh[0] + 1):
        for ky in range(-nsh[1], nsh[1] + 1):
            for kz in range(-nsh[2], nsh[2] + 1):
                s = kx * h[:, 0] + ky * h[:, 1] + kz * h[:, 2]
                xj = x + s
                keep = np.nonzero(np.all((xj > lo - rmax) & (xj < hi + rmax), axis=1))[0]
                if not len(keep):
                    continue
                xj = xj[keep]
                own = kx == 0 and ky == 0 and kz == 0
                for i0 in range(0, n, 512):
                    i1 = min(i0 + 512, n)
                    d = xj[None, :, :] - x[i0:i1, None, :]
                    rsq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
                    hit = rsq < rmax * rmax
                    if own:
                        hit &= keep[None, :] != np.arange(i0, i1)[:, None]
                    a, b = np.nonzero(hit)
                    if len(a):
                        out.append((a + i0, keep[b], d[a, b], rsq[a, b]))
    if not out:
        return np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros((0, 3)), np.zeros(0)
    i, j, d, rsq = (np.concatenate([o[k] for o in out]) for k in range(4))
    order = np.argsort(i, kind="stable")
    return i[order], j[order], d[order], rsq[order]


def ordinate_of(c, ordinate):
    c = np.clip(c, -1.0, 1.0)
    if ordinate == "cosine":
        return c
    return np.arccos(c) * (180.0 / math.pi) if ordinate == "degree" else np.arccos(c)


def counts(x, types, h, periodic, nbin, ordinate, triples, member=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    types = np.asarray(types)
    h = np.asarray(h, dtype=np.float64)
    n, ntr = len(x), len(triples)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member).astype(bool)
    lo, hi = RANGE[ordinate]
    in_i = np.array([(types >= t[0]) & (types <= t[1]) & member for t in triples])
    in_j = np.array([(types >= t[2]) & (types <= t[3]) & member for t in triples])
    in_k = np.array([(types >= t[4]) & (types <= t[5]) & member for t in triples])
    rmax = max(max(t[7], t[9]) for t in triples)
    ni, nj, nd, nrsq = neighbours(x, h, periodic, rmax * (1.0 + 1e-6))
    radii = sorted({float(r) for t in triples for r in t[6:10] if r > 0.0})
    near_shell = np.zeros(len(nrsq), dtype=bool)
    for r in radii:
        near_shell |= np.abs(nrsq - r * r) <= 1e-9 * r * r
    n_shell_edge = int((near_shell & in_i.any(axis=0)[ni] & member[nj]).sum())
    hist = np.zeros((ntr, nbin), dtype=np.int64)
    sure = np.zeros((ntr, nbin), dtype=np.int64)
    adjacent = np.zeros((ntr, nbin), dtype=np.int64)
    n_edge = 0
    start = np.searchsorted(ni, np.arange(n + 1))
    centres = np.nonzero(in_i.any(axis=0))[0]
    for i in centres:
        a0, a1 = start[i], start[i + 1]
        if a1 - a0 < 2:
            continue
        j, d, rsq = nj[a0:a1], nd[a0:a1], nrsq[a0:a1]
        r = np.sqrt(rsq)
        c = (d @ d.T) / (r[:, None] * r[None, :])
        t = (ordinate_of(c, ordinate) - lo) * nbin / (hi - lo)
        near = np.rint(t)
        is_edge = (np.abs(t - near) < EDGE) & (near > 0) & (near < nbin)
        b = np.minimum(t.astype(np.int64), nbin - 1)
        off = ~np.eye(len(j), dtype=bool)
        any_edge = np.zeros_like(off)
        for m in np.nonzero(in_i[:, i])[0]:
            tr = triples[m]
            jq = in_j[m, j] & (rsq >= tr[6] * tr[6]) & (rsq < tr[7] * tr[7])
            kq = in_k[m, j] & (rsq >= tr[8] * tr[8]) & (rsq < tr[9] * tr[9])
            sel = jq[:, None] & kq[None, :] & off
            if not sel.any():
                continue
            hist[m] += np.bincount(b[sel], minlength=nbin)
            sure[m] += np.bincount(b[sel & ~is_edge], minlength=nbin)
            e = sel & is_edge
            if e.any():
                any_edge |= e
                for bb in near[e].astype(np.int64):
                    adjacent[m, bb - 1] += 1
                    adjacent[m, bb] += 1
        n_edge += int(any_edge.sum())
    return dict(hist=hist, hist_sure=sure, edge_adjacent=adjacent, n_edge=n_edge, icount=in_i.sum(axis=1).astype(np.int64),
                n_shell_edge=n_shell_edge, max_neighbours=int(np.diff(np.searchsorted(ni[nrsq < rmax * rmax], np.arange(n + 1))).max(initial=0)))


def normalise(hist, icount, nbin, ordinate="degree", cumulative="fraction"):
    """the compute's array, loop for loop: [nbin][1 + 2 ntriple] = bin centre, then hist / (count delta) and the running sum
    of hist over count (fraction) or over icount (centre) per triple"""
    hist = np.atleast_2d(hist)
    lo, hi = RANGE[ordinate]
    delta = (hi - lo) / nbin
    out = np.zeros((nbin, 1 + 2 * len(hist)))
    for b in range(nbin):
        out[b, 0] = lo + (b + 0.5) * delta
    for m in range(len(hist)):
        count = float(hist[m].sum())
        den = count if cumulative == "fraction" else float(icount[m])
        run = 0.0
        for b in range(nbin):
            run += float(hist[m, b])
            out[b, 1 + 2 * m] = float(hist[m, b]) / (count * delta) if count > 0 else 0.0
            out[b, 2 + 2 * m] = run / den if den > 0 else 0.0
    return out


def check_inputs(ref, max_edge=2):
    """conditions on the inputs, not measurements: at most max_edge angles at a bin edge, no neighbour at a shell radius"""
    assert ref["n_edge"] <= max_edge, ref["n_edge"]
    assert ref["n_shell_edge"] == 0, ref["n_shell_edge"]


def check_bracket(dev_hist, ref, max_edge=2):
    """the device histogram lies in the reference's bracket, and the reference's inputs satisfy check_inputs"""
    dev_hist = np.atleast_2d(dev_hist)
    check_inputs(ref, max_edge)
    low, high = ref["hist_sure"], ref["hist_sure"] + ref["edge_adjacent"]
    bad = np.argwhere((dev_hist < low) | (dev_hist > high))
    assert len(bad) == 0, [(int(m), int(b), int(dev_hist[m, b]), int(low[m, b]), int(high[m, b])) for m, b in bad[:8]]
