"""CPU: tests/heatfluxref.py, the NumPy reference of the heat current, against a three-atom case worked out by hand and
against the identities the formula implies."""
import numpy as np

import heatfluxref


def test_three_atoms_by_hand():
    """mvv2e = 2 makes ke = m v.v.
    atom 1: m 1, v (1, 0, 0),  pe 0.5,  W xx = 2                    -> ke 1, e 1.5; conv (1.5, 0, 0);  W.v (2, 0, 0)
    atom 2: m 2, v (0, 2, -1), pe -1,   W (yy 1, zz 3, xy 4, yz -2) -> ke 10, e 9;  conv (0, 18, -9);  W.v (8, 2+2, -4-3) = (8, 4, -7)
    atom 3: m 3, v (-1, 1, 1), pe 0,    W (xz 5)                    -> ke 9, e 9;   conv (-9, 9, 9);   W.v (5, 0, -5)"""
    mass = [1.0, 2.0, 3.0]
    v = [[1.0, 0.0, 0.0], [0.0, 2.0, -1.0], [-1.0, 1.0, 1.0]]
    pe = [0.5, -1.0, 0.0]
    w = [[2.0, 0, 0, 0, 0, 0], [0, 1.0, 3.0, 4.0, 0, -2.0], [0, 0, 0, 0, 5.0, 0]]
    r = heatfluxref.sums(mass, v, pe, w, 2.0)
    assert r["sums"].tolist() == [-7.5, 27.0, 0.0, 15.0, 4.0, -12.0, 3.0, 19.5]
    assert r["mag"].tolist() == [10.5, 27.0, 18.0, 15.0, 4.0, 12.0, 3.0, 19.5]
    assert r["vector"].tolist() == [7.5, 31.0, -12.0, -7.5, 27.0, 0.0]
    g = heatfluxref.sums(mass, v, pe, w, 2.0, member=[True, False, True])
    assert g["sums"].tolist() == [-7.5, 9.0, 9.0, 7.0, 0.0, -5.0, 2.0, 10.5]


def test_without_potential_terms_it_is_the_kinetic_energy_current():
    rng = np.random.default_rng(5)
    n, mvv2e = 200, 1.0364269e-4
    mass, v = rng.uniform(20.0, 100.0, n), rng.normal(0.0, 3.0, (n, 3))
    r = heatfluxref.sums(mass, v, np.zeros(n), np.zeros((n, 6)), mvv2e)
    ke = 0.5 * mvv2e * mass * (v ** 2).sum(axis=1)
    want = (ke[:, None] * v).sum(axis=0)
    assert np.allclose(r["sums"][0:3], want, rtol=1e-13, atol=0.0)
    assert np.array_equal(r["sums"][3:6], np.zeros(3)) and np.array_equal(r["vector"][:3], r["vector"][3:])
    assert r["sums"][6] == n and abs(r["sums"][7] - ke.sum()) <= 1e-13 * ke.sum()
    assert np.all(r["mag"][0:3] >= np.abs(r["sums"][0:3]))


def test_the_virial_part_is_linear_and_symmetric():
    """W.v with W built from one symmetric 3 x 3 matrix per atom equals the matrix product"""
    rng = np.random.default_rng(6)
    n = 50
    a = rng.normal(size=(n, 3, 3))
    sym = a + a.transpose(0, 2, 1)
    w = np.stack([sym[:, 0, 0], sym[:, 1, 1], sym[:, 2, 2], sym[:, 0, 1], sym[:, 0, 2], sym[:, 1, 2]], axis=1)
    v = rng.normal(size=(n, 3))
    r = heatfluxref.sums(np.ones(n), v, np.zeros(n), w, 0.0)
    assert np.allclose(r["sums"][3:6], np.einsum("nij,nj->i", sym, v), rtol=1e-12, atol=1e-12)
    assert np.array_equal(r["sums"][0:3], np.zeros(3))
