"""CPU: tests/rdfref.py -- the NumPy brute force the GPU tests of compute rdf/mdp are read against -- on cases whose answers
are known without it, and resident.rdf_normalise against the reference's loop-for-loop normalisation."""
import itertools
import math

import numpy as np

from lammps_plugins_amd.host import resident, system as S
import rdfref

PER = (1, 1, 1)


def test_fcc_shells():
    """a perfect 6 x 6 x 6 fcc lattice, a = 4.045 A: the coordination column steps through 12, 18, 42, 54 at the shell
    radii a / sqrt 2, a, a sqrt(3/2), a sqrt 2.  44 bins below 5.8 A put the shells 0.70, 0.69, 0.58 and 0.40 of a bin above
    a bin edge (asserted: at least a quarter from both edges), so no lattice distance is an edge pair."""
    a, nbin, cutoff = 4.045, 44, 5.8
    s = S.fcc_cell(a, 6)
    shells = [a / math.sqrt(2.0), a, a * math.sqrt(1.5), a * math.sqrt(2.0)]
    assert a * math.sqrt(2.5) > cutoff
    at = [r * nbin / cutoff for r in shells]
    assert all(0.25 <= t % 1.0 <= 0.75 for t in at), at
    ref = rdfref.rdf(s.x, s.type, s.box.h, PER, cutoff, nbin, [(1, 1, 1, 1)])
    assert ref["n_edge"] == 0 and not ref["edge_adjacent"].any()
    assert np.array_equal(ref["hist"], ref["hist_sure"])
    g, coord = ref["array"][:, 1], ref["array"][:, 2]
    bins = [int(t) for t in at]
    want = np.zeros(nbin)
    for b, c in zip(bins, (12, 18, 42, 54)):
        want[b:] = c
    assert np.allclose(coord, want, rtol=0, atol=1e-9)
    assert np.all(g[[b for b in range(nbin) if b not in bins]] == 0.0) and np.all(g[bins] > 0.0)
    assert np.array_equal(ref["hist"][0][bins], np.array([12, 6, 24, 12]) * s.n)
    assert np.allclose(ref["array"][:, 0], (np.arange(nbin) + 0.5) * cutoff / nbin, rtol=1e-15)
    mine = resident.rdf_normalise(ref["hist"], ref["icount"], ref["jcount"], ref["dup"], cutoff, s.box.volume)
    assert np.allclose(mine, ref["array"], rtol=1e-13, atol=1e-13)


def test_uniform_points_have_g_one():
    """20 000 uniform random points at unit density: an ordered-pair bin count is twice a Poisson count of mean mu / 2
    (mu = N normfac vfrac), so its standard deviation is sqrt(2 mu); g = count / mu is 1 within 5 of them for r above
    two bins"""
    n, nbin, cutoff = 20000, 25, 2.5
    edge = n ** (1.0 / 3.0)
    rng = np.random.default_rng(20261018)
    x = rng.random((n, 3)) * edge
    h = np.diag([edge] * 3)
    ref = rdfref.rdf(x, np.ones(n, dtype=np.int32), h, PER, cutoff, nbin, [(1, 1, 1, 1)])
    delr = cutoff / nbin
    b = np.arange(nbin)
    mu = n * (n - 1.0) * 4.0 * math.pi / (3.0 * edge ** 3) * (((b + 1) * delr) ** 3 - (b * delr) ** 3)
    g = ref["array"][:, 1]
    assert np.allclose(g, ref["hist"][0] / mu, rtol=1e-12)
    assert np.all(np.abs(g - 1.0)[2:] <= 5.0 * np.sqrt(2.0 / mu)[2:]), (g, 5.0 * np.sqrt(2.0 / mu))
    assert ref["hist"][0].sum() % 2 == 0 and ref["hist"][0][2:].min() > 1000


def test_two_types_cross_pairs_and_hand_counts():
    """8 atoms, types 1 1 1 2 2 1 2 1 (five of type 1, three of type 2), at random places in a 5 A box with a 4 A cutoff:
    the 1-2 and 2-1 columns hold the same counts (an ordered pair read from either end), icount / jcount / dup and normfac
    are the hand counts, and a group that leaves atoms out counts the members only"""
    types = np.array([1, 1, 1, 2, 2, 1, 2, 1], dtype=np.int32)
    rng = np.random.default_rng(5)
    x = rng.random((8, 3)) * 5.0
    h = np.diag([5.0] * 3)
    pairs = [(1, 1, 1, 1), (1, 1, 2, 2), (2, 2, 1, 1), (2, 2, 2, 2), (1, 2, 1, 2), (1, 1, 1, 2)]
    ref = rdfref.rdf(x, types, h, PER, 4.0, 16, pairs)
    assert np.array_equal(ref["hist"][1], ref["hist"][2]) and ref["hist"][1].sum() > 0
    assert np.array_equal(ref["hist"][0] + ref["hist"][1] + ref["hist"][2] + ref["hist"][3], ref["hist"][4])
    assert np.array_equal(ref["hist"][0] + ref["hist"][1], ref["hist"][5])
    assert ref["icount"].tolist() == [5, 5, 3, 3, 8, 5]
    assert ref["jcount"].tolist() == [5, 3, 5, 3, 8, 8]
    assert ref["dup"].tolist() == [5, 0, 0, 3, 8, 5]
    # normfac = jcount - dup / icount: 4, 3, 5, 2, 7, 7; the last coordination number is pairs per i atom
    for m, normfac in enumerate((4.0, 3.0, 5.0, 2.0, 7.0, 7.0)):
        assert math.isclose(ref["array"][-1, 2 + 2 * m], ref["hist"][m].sum() / ref["icount"][m], rel_tol=1e-12)
        delr, const = 4.0 / 16, 4.0 * math.pi / (3.0 * 125.0)
        vfrac = const * (16 ** 3 - 15 ** 3) * delr ** 3
        assert math.isclose(ref["array"][-1, 1 + 2 * m], ref["hist"][m][-1] / (vfrac * normfac * ref["icount"][m]), rel_tol=1e-12)
    member = np.array([1, 0, 1, 1, 0, 1, 1, 1], dtype=bool)
    grp = rdfref.rdf(x, types, h, PER, 4.0, 16, pairs, member)
    sub = rdfref.rdf(x[member], types[member], h, PER, 4.0, 16, pairs)
    assert np.array_equal(grp["hist"], sub["hist"]) and grp["icount"].tolist() == [4, 4, 2, 2, 6, 4]
    assert np.array_equal(grp["dup"], sub["dup"]) and np.array_equal(grp["jcount"], sub["jcount"])


def test_triclinic_box_shorter_than_the_cutoff_counts_self_images():
    """two atoms in a sheared cell with edges of 3, 4 and 11 A and a 7.5 A cutoff: the partners of an atom are lattice
    points, its own images among them; against a direct enumeration of the lattice sums"""
    h = np.array([[3.0, -1.2, 0.4], [0.0, 4.0, 0.9], [0.0, 0.0, 11.0]])
    x = np.array([[0.3, 0.2, 0.5], [1.7, 2.9, 6.1]])
    cutoff, nbin = 7.5, 30
    ref = rdfref.rdf(x, np.array([1, 2]), h, PER, cutoff, nbin, [(1, 1, 1, 1), (1, 1, 2, 2), (1, 2, 1, 2)])
    want = np.zeros((3, nbin), dtype=np.int64)
    for k in itertools.product(range(-6, 7), repeat=3):
        s = k[0] * h[:, 0] + k[1] * h[:, 1] + k[2] * h[:, 2]
        for i, j in itertools.product(range(2), repeat=2):
            if i == j and k == (0, 0, 0):
                continue
            b = int(np.linalg.norm(x[i] - x[j] - s) * nbin / cutoff)
            if b < nbin:
                want[2, b] += 1
                if i == 0:
                    want[0 if j == 0 else 1, b] += 1
    assert np.array_equal(ref["hist"], want)
    assert want[0].sum() >= 12 and want[0][:int(3.0 * nbin / cutoff)].sum() == 0 and want[0][int(3.0 * nbin / cutoff)] == 2
    # not periodic along z: the images along the 11 A edge are gone, the others stay
    slab = rdfref.rdf(x, np.array([1, 2]), h, (1, 1, 0), cutoff, nbin, [(1, 2, 1, 2)])
    assert 0 < slab["hist"][0].sum() < want[2].sum()
