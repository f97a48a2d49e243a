"""NumPy reference of LAMMPS compute rdf for the tests of compute rdf/mdp: a brute force over every atom pair and every
periodic image, in integers, with LAMMPS' normalisation on top.

counts(x, types, h, periodic, cutoff, nbin, pairs, member): x[n][3] and types[n] by tag (row t - 1 = the atom with tag t), h
the 3 x 3 box matrix whose COLUMNS are the box vectors (system.Box.h), periodic three flags, pairs a list of
(ilo, ihi, jlo, jhi) inclusive type ranges, member[n] booleans by tag or None.  An ordered pair (i, j + image) counts when
both atoms are members, the types fit the column, and (int) (r nbin / cutoff) < nbin; (j, image) = (i, no shift) is the
one entry left out: an atom's own periodic image is a partner like any other, as LAMMPS' ghost atoms are.  Every image
shift whose box vectors can reach inside the cutoff is visited (not just -1 .. 1: a box edge may be shorter than the
cutoff, and atoms may sit a little outside the box).

A device that forms the same r up to its last bit puts a pair into another bin only if r nbin / cutoff is within
rounding of an integer.  So every in-range pair is classed as SURE (r nbin / cutoff at least EDGE = 1e-9 away from every
integer) or EDGE (closer than that to a bin edge or to the cutoff); a device histogram is right when, for every column
and bin, hist_sure <= device <= hist_sure + edge_adjacent.  The tests also cap the number of edge pairs.

The only shortcut is the order of the work: atoms are sorted by x, and a block of rows is compared with the atoms whose
(shifted) x lies within the cutoff of the block's x range, images that lie beyond the cutoff of the atoms' bounding box
left out beforehand -- every pair within the cutoff is still met, tested on its
full distance."""
import math

import numpy as np

EDGE = 1e-9


def _shift_ranges(x, h, periodic, cutoff):
    hinv = np.linalg.inv(h)
    lam = x @ hinv.T
    span = lam.max(axis=0) - lam.min(axis=0)
    out = []
    for d in range(3):
        if not periodic[d]:
            out.append(0)
            continue
        width = 1.0 / np.linalg.norm(hinv[d])        # perpendicular width of the box along lamda_d
        out.append(int(math.floor(span[d] + cutoff / width + 1e-9)))
    return out


def _pairs_in_range(x, h, periodic, rmax):
    """yields (i, j, r) arrays of every ordered pair (i, j + image) with r < rmax, (j, image) != (i, 0)"""
    n = len(x)
    order = np.argsort(x[:, 0], kind="stable")
    xs = x[order]
    nsh = _shift_ranges(x, h, periodic, rmax)
    lo, hi = x.min(axis=0), x.max(axis=0)
    block = 256
    for kx in range(-nsh[0], nsh[0] + 1):
        for ky in range(-nsh[1], nsh[1] + 1):
            for kz in range(-nsh[2], nsh[2] + 1):
                s = kx * h[:, 0] + ky * h[:, 1] + kz * h[:, 2]
                gap = np.maximum(0.0, np.maximum(lo - (hi + s), (lo + s) - hi))   # between the two bounding boxes
                if float((gap * gap).sum()) >= rmax * rmax:
                    continue
                own = kx == 0 and ky == 0 and kz == 0
                xj, oj = xs + s, order                        # (still sorted by x: the shift is the same for all)
                if not own:                                   # the images that can reach the atoms at all
                    keep = np.all((xj > lo - rmax) & (xj < hi + rmax), axis=1)
                    xj, oj = xj[keep], order[keep]
                    if not len(xj):
                        continue
                for i0 in range(0, n, block):
                    i1 = min(i0 + block, n)
                    j0 = int(np.searchsorted(xj[:, 0], xs[i0, 0] - rmax, side="left"))
                    j1 = int(np.searchsorted(xj[:, 0], xs[i1 - 1, 0] + rmax, side="right"))
                    if j1 <= j0:
                        continue
                    dx = xs[i0:i1, None, 0] - xj[None, j0:j1, 0]
                    dy = xs[i0:i1, None, 1] - xj[None, j0:j1, 1]
                    dz = xs[i0:i1, None, 2] - xj[None, j0:j1, 2]
                    rsq = dx * dx + dy * dy + dz * dz
                    hit = rsq < rmax * rmax
                    if own:
                        ii = np.arange(i0, i1)
                        inside = (ii >= j0) & (ii < j1)
                        hit[ii[inside] - i0, ii[inside] - j0] = False
                    a, b = np.nonzero(hit)
                    if len(a):
                        yield order[a + i0], oj[b + j0], np.sqrt(rsq[a, b])


def counts(x, types, h, periodic, cutoff, nbin, pairs, member=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    types = np.asarray(types)
    h = np.asarray(h, dtype=np.float64)
    n, npair = len(x), len(pairs)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member).astype(bool)
    in_i = np.array([(types >= p[0]) & (types <= p[1]) & member for p in pairs])
    in_j = np.array([(types >= p[2]) & (types <= p[3]) & member for p in pairs])
    hist = np.zeros((npair, nbin), dtype=np.int64)
    sure = np.zeros((npair, nbin), dtype=np.int64)
    adjacent = np.zeros((npair, nbin), dtype=np.int64)
    n_edge = 0
    for i, j, r in _pairs_in_range(x, h, periodic, cutoff * (1.0 + 1e-6)):
        t = r * nbin / cutoff
        near = np.rint(t)
        is_edge = np.abs(t - near) < EDGE
        b = t.astype(np.int64)
        for k in np.nonzero(is_edge)[0]:                      # (rare: a handful at the most)
            for m in range(npair):
                if in_i[m, i[k]] and in_j[m, j[k]]:
                    for bb in (int(near[k]) - 1, int(near[k])):
                        if 0 <= bb < nbin:
                            adjacent[m, bb] += 1
            if member[i[k]] and member[j[k]]:
                n_edge += 1
        ok = b < nbin
        for m in range(npair):
            sel = ok & in_i[m, i] & in_j[m, j]
            hist[m] += np.bincount(b[sel], minlength=nbin)[:nbin]
            sel &= ~is_edge
            sure[m] += np.bincount(b[sel], minlength=nbin)[:nbin]
    icount = in_i.sum(axis=1).astype(np.int64)
    jcount = in_j.sum(axis=1).astype(np.int64)
    dup = (in_i & in_j).sum(axis=1).astype(np.int64)
    return dict(hist=hist, hist_sure=sure, edge_adjacent=adjacent, n_edge=n_edge, icount=icount, jcount=jcount, dup=dup)


def normalise(hist, icount, jcount, dup, cutoff, volume):
    """LAMMPS' ComputeRDF::compute_array, loop for loop: [nbin][1 + 2 npair] = bin centre, then g(r) and coord per pair"""
    hist = np.atleast_2d(hist)
    npair, nbin = hist.shape
    delr = cutoff / nbin
    constant = 4.0 * math.pi / (3.0 * volume)
    out = np.zeros((nbin, 1 + 2 * npair))
    for b in range(nbin):
        out[b, 0] = (b + 0.5) * delr
    for m in range(npair):
        ic, jc, du = float(icount[m]), float(jcount[m]), float(dup[m])
        normfac = jc - du / ic if ic > 0 else 0.0
        ncoord = 0.0
        for b in range(nbin):
            rlower, rupper = b * delr, (b + 1) * delr
            vfrac = constant * (rupper ** 3 - rlower ** 3)
            den = vfrac * normfac * ic
            gr = float(hist[m, b]) / den if den != 0.0 else 0.0
            ncoord += gr * vfrac * normfac
            out[b, 1 + 2 * m] = gr
            out[b, 2 + 2 * m] = ncoord
    return out


def rdf(x, types, h, periodic, cutoff, nbin, pairs, member=None):
    """counts() plus the normalised array (from hist, with edge pairs where NumPy's r puts them)"""
    c = counts(x, types, h, periodic, cutoff, nbin, pairs, member)
    prd = np.asarray(h, dtype=np.float64).diagonal()
    c["array"] = normalise(c["hist"], c["icount"], c["jcount"], c["dup"], cutoff, float(prd[0] * prd[1] * prd[2]))
    return c


def check_bracket(dev_hist, ref, max_edge=2):
    """the device histogram lies in the reference's bracket, and the reference saw at most max_edge edge pairs"""
    dev_hist = np.atleast_2d(dev_hist)
    assert ref["n_edge"] <= max_edge, ref["n_edge"]
    low, high = ref["hist_sure"], ref["hist_sure"] + ref["edge_adjacent"]
    bad = np.argwhere((dev_hist < low) | (dev_hist > high))
    assert len(bad) == 0, [(int(m), int(b), int(dev_hist[m, b]), int(low[m, b]), int(high[m, b])) for m, b in bad[:8]]
