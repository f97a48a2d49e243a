"""NumPy reference of compute cna/atom/mdp (LAMMPS compute cna/atom Rc) for its tests: a brute force over every atom pair and
every periodic image on adfref.neighbours, and the constructed cells the tests share.

x[n][3] is by tag (row t - 1 = the atom with tag t), h the 3 x 3 box matrix whose COLUMNS are the box vectors
(system.Box.h), periodic three flags, member[n] booleans by tag or None: the CENTRES.  A neighbour is any other entry (atom,
image) of any group, the centre's own images included, with rsq < cutoff^2 (include/mdpair_hip.h, mdp_cna_read).

cna(...) returns dict(pattern[n], neighbours[n], ambiguous[n]): 1 fcc, 2 hcp, 3 bcc, 4 icosahedral, 5 other, 0 outside the
group; the number of neighbours; and whether any distance the atom's answer uses lies within EDGE = rdfref.EDGE = 1e-9
relative of cutoff^2 -- centre to candidate, and, where the atom has 12 or 14 neighbours, neighbour to neighbour.  Neighbour
to neighbour distances are formed from the difference of the two displacements from the centre, as the device forms them;
the device compiles with -ffp-contract=fast, so the last bit of an rsq may differ from NumPy's and nothing else: only a
distance within rounding of the cutoff can be decided differently, and the tests compare every atom that has none."""
import numpy as np

import adfref
import rdfref

EDGE = rdfref.EDGE
FCC, HCP, BCC, ICO, OTHER = 1, 2, 3, 4, 5
MINBOND_EMPTY = 8                      # LAMMPS initialises minbond with MAXCOMMON


def signature(adj, m):
    """(ncommon, nbonds, maxbond, minbond) of bond m from the boolean adjacency of the centre's neighbours (no diagonal)"""
    common = np.nonzero(adj[m])[0]
    if not len(common):
        return 0, 0, 0, MINBOND_EMPTY
    bonds = adj[np.ix_(common, common)].sum(axis=1)
    return len(common), int(bonds.sum()) // 2, int(bonds.max()), min(int(bonds.min()), MINBOND_EMPTY)


def pattern_of(sigs):
    """the pattern of a centre from the signatures of its 12 or 14 bonds"""
    count = lambda s: sum(1 for t in sigs if t == s)
    if len(sigs) == 12:
        if count((4, 2, 1, 1)) == 12:
            return FCC
        if count((4, 2, 1, 1)) == 6 and count((4, 2, 2, 0)) == 6:
            return HCP
        if count((5, 5, 2, 2)) == 12:
            return ICO
    if len(sigs) == 14 and count((4, 4, 2, 2)) == 6 and count((6, 6, 2, 2)) == 8:
        return BCC
    return OTHER


def cna(x, h, periodic, cutoff, member=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = len(x)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member).astype(bool)
    cutsq = cutoff * cutoff
    i, j, d, rsq = adfref.neighbours(x, h, periodic, cutoff * (1.0 + 1e-6))      # (candidates: a hair past the cutoff)
    start = np.searchsorted(i, np.arange(n + 1))
    pattern, nn, amb = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for k in range(n):
        dk, rk = d[start[k]:start[k + 1]], rsq[start[k]:start[k + 1]]
        inside = rk < cutsq
        nn[k] = int(inside.sum())
        if not member[k]:
            continue
        amb[k] = bool(np.any(np.abs(rk / cutsq - 1.0) < EDGE))
        pattern[k] = OTHER
        if nn[k] not in (12, 14):
            continue
        u = dk[inside]
        w = u[:, None, :] - u[None, :, :]
        wsq = w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2]
        off = ~np.eye(len(u), dtype=bool)
        amb[k] |= bool(np.any((np.abs(wsq / cutsq - 1.0) < EDGE) & off))
        adj = (wsq < cutsq) & off
        pattern[k] = pattern_of([signature(adj, m) for m in range(len(u))])
    return dict(pattern=pattern, neighbours=nn, ambiguous=amb)


def histogram(pattern):
    """int64[6]: the atoms of pattern 0 .. 5"""
    return np.bincount(np.asarray(pattern).astype(np.int64), minlength=6)[:6]


# ---- the constructed cells: (x[n][3], h[3][3]); the jitter is sigma times standard normal deviates of default_rng(seed)
A_FCC, A_BCC = 4.045, 3.302
RC_FCC, RC_BCC = 0.8536 * A_FCC, 1.2071 * A_BCC
STACK = "ABCABCABABAB"                 # layers 1 .. 6 have unlike layers below and above (fcc), layers 0 and 7 .. 11 like ones (hcp)
ICO_RADIUS, ICO_BOX = 2.86, 24.27
RC_ICO = 1.35 * ICO_RADIUS


def _jitter(x, sigma, seed):
    return x + sigma * np.random.default_rng(seed).standard_normal(x.shape) if sigma > 0.0 else x


def fcc_cell(ncell=6, sigma=0.0, seed=1, gone=None):
    """4 ncell^3 atoms of fcc with a = 4.045 A in the order of system.fcc_cell, without row `gone` if given"""
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    k, j, i = np.meshgrid(np.arange(ncell), np.arange(ncell), np.arange(ncell), indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * A_FCC
    if gone is not None:
        x = x[np.arange(len(x)) != gone]
    return _jitter(x, sigma, seed), np.diag([ncell * A_FCC] * 3)


def stack_cell(sigma=0.05, seed=1, nx=8, ny=5):
    """close-packed layers in the sequence STACK, 2 nx ny atoms each at the nearest-neighbour distance of the fcc cell, in an
    orthorhombic box: 960 atoms in 22.88 x 24.77 x 28.02 A.  Returns (x, h, layer[n])"""
    d = A_FCC / np.sqrt(2.0)
    ax, ay, az = d, d * np.sqrt(3.0), d * np.sqrt(2.0 / 3.0)
    shift = dict(A=(0.0, 0.0), B=(0.5 * ax, ay / 6.0), C=(0.0, ay / 3.0))
    xs, layer = [], []
    for l, s in enumerate(STACK):
        for j in range(ny):
            for i in range(nx):
                for bx, by in ((0.0, 0.0), (0.5, 0.5)):
                    xs.append(((i + bx) * ax + shift[s][0], (j + by) * ay + shift[s][1], l * az))
                    layer.append(l)
    return _jitter(np.array(xs), sigma, seed), np.diag([nx * ax, ny * ay, len(STACK) * az]), np.array(layer)


def stack_lattice(origin=(0.1, 0.1, 0.02)):
    """the stack as a LAMMPS `lattice custom` command: one orthorhombic cell of 24 basis atoms, two per layer; `region block 0 nx
    0 ny 0 1` of it is stack_cell(0.0, nx=nx, ny=ny) shifted by the origin"""
    d = A_FCC / np.sqrt(2.0)
    frac = dict(A=(0.0, 0.0), B=(0.5, 1.0 / 6.0), C=(0.0, 1.0 / 3.0))
    words = ["lattice custom 1.0", "a1 %.17g 0.0 0.0" % d, "a2 0.0 %.17g 0.0" % (d * np.sqrt(3.0)),
             "a3 0.0 0.0 %.17g" % (len(STACK) * d * np.sqrt(2.0 / 3.0))]
    for l, s in enumerate(STACK):
        for bx, by in ((0.0, 0.0), (0.5, 0.5)):
            words.append("basis %.17g %.17g %.17g" % ((bx + frac[s][0]) % 1.0, (by + frac[s][1]) % 1.0, l / len(STACK)))
    words.append("origin %g %g %g" % tuple(origin))
    return " &\n    ".join(words)


def bcc_cell(ncell=8, sigma=0.04, seed=1):
    """2 ncell^3 atoms of bcc with a = 3.302 A"""
    k, j, i = np.meshgrid(np.arange(ncell), np.arange(ncell), np.arange(ncell), indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(float)
    x = (cells[:, None, :] + np.array([[0, 0, 0], [0.5, 0.5, 0.5]])[None, :, :]).reshape(-1, 3) * A_BCC
    return _jitter(x, sigma, seed), np.diag([ncell * A_BCC] * 3)


def icosahedron_cell(sigma=0.03, seed=1):
    """an atom in the middle of a periodic cube of 24.27 A (row 0) and twelve at the vertices of an icosahedron of radius 2.86 A"""
    phi = 0.5 * (1.0 + np.sqrt(5.0))
    v = [(0.0, s1, s2 * phi) for s1 in (-1.0, 1.0) for s2 in (-1.0, 1.0)]
    v = np.array([p[r:] + p[:r] for p in v for r in range(3)])
    v *= ICO_RADIUS / np.sqrt(1.0 + phi * phi)
    x = np.concatenate([np.zeros((1, 3)), v]) + 0.5 * ICO_BOX
    return _jitter(x, sigma, seed), np.diag([ICO_BOX] * 3)
