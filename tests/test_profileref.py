"""CPU: tests/profileref.py against a slow per-atom loop; resident.profile_normalise against the reference's; the two-halves
split that carries an int64 through a sum of doubles; and the exponent rule of mdp_profile_exponent (the library's one copy,
a pure host function) against the reference's and against the bound it promises."""
import math
from fractions import Fraction

import numpy as np
import pytest

from lammps_plugins_amd.host import capi, resident, system as S
import profileref


def _atoms(n=700, seed=5):
    rng = np.random.default_rng(seed)
    lam = rng.uniform(-0.3, 1.3, size=(n, 3))          # some atoms outside the box on every side
    mass = rng.choice([26.98, 28.09, 95.94], size=n)
    v = rng.normal(0.0, 7.0, size=(n, 3))
    return lam, mass, v


@pytest.mark.parametrize("dims,nbins,periodic", [
    ((2,), (7,), (True, True, True)),
    ((0, 1), (5, 11), (True, True, False)),
    ((2, 0, 1), (3, 4, 5), (True, False, False)),
    ((1,), (1,), (False, False, False)),
])
def test_table_against_a_per_atom_loop(dims, nbins, periodic):
    lam, mass, v = _atoms()
    member = np.arange(len(lam)) % 3 != 0
    ref = profileref.table(lam, periodic, dims, nbins, mass, v, member=member)
    rows = int(np.prod(nbins))
    count, sums = [0] * rows, [[0] * 5 for _ in range(rows)]
    exact = [[Fraction(0) for _ in range(5)] for _ in range(rows)]
    for i in range(len(lam)):
        if not member[i]:
            continue
        row = 0
        for d, n in zip(dims, nbins):
            b = math.floor(lam[i, d] * n)
            b = b % n if periodic[d] else min(max(b, 0), n - 1)
            row = row * n + b
        m, (vx, vy, vz) = float(mass[i]), (float(c) for c in v[i])
        t = (m, m * vx, m * vy, m * vz, m * (vx * vx + vy * vy + vz * vz))
        count[row] += 1
        for k in range(5):
            sums[row][k] += round(math.ldexp(t[k], int(ref["exponents"][k])))    # (round half to even, as rint)
            exact[row][k] += Fraction(t[k])
    assert ref["count"].tolist() == count and ref["sums"].tolist() == sums
    assert all(ref["exact"][b][k] == float(exact[b][k]) for b in range(rows) for k in range(5))
    assert ref["count"].sum() == member.sum() and ref["n_edge"] == 0
    # the reference passes its own check, and the quantised sums are close to the exact ones, not equal to them
    assert 0.0 < profileref.check_sums(ref["count"], ref["sums"], ref["exponents"], ref) <= 0.5
    # the exponents leave 2^61 / N of headroom: the largest quantised term is within a factor 2 of it
    n2 = 2 ** (len(lam) - 1).bit_length()
    q = np.abs(np.rint(np.ldexp(profileref.terms(mass, v)[member], ref["exponents"]))).max(axis=0)
    assert np.all(q < 2.0 ** 61 / n2) and np.all(q >= 2.0 ** 60 / n2)


def test_edge_atoms_are_counted():
    lam = np.array([[0.5, 0.25, 0.1], [0.5 + 1e-12, 0.3, 0.2], [0.31, 0.3, 0.4]])
    assert profileref.bins(lam, (True,) * 3, (0,), (4,))[1] == 2
    assert profileref.bins(lam, (True,) * 3, (0,), (3,))[1] == 0
    assert profileref.bins(lam, (True,) * 3, (2, 1), (3, 4))[1] == 1


def test_check_sums_with_edges_brackets_the_rows_of_an_edge_atom_and_no_other():
    """three atoms planted at bin edges of a (4, 3) grid over (0, 2) -- one at an x edge, one at a z edge, one at a corner, a
    periodic face among them --: the rows either side of each edge are bracketed, every other row stays exact; a table in
    which the planted atoms sit on the other side passes, one with an atom moved between sure rows, or with a sum of a sure
    row off by more than its bound, does not; without edge atoms the variant is check_sums"""
    lam, mass, v = _atoms(seed=11)
    lam[0], lam[1], lam[2] = (0.5 - 1e-12, 0.3, 0.2), (0.1, 0.3, 2.0 / 3.0 + 1e-12), (1.0 - 1e-12, 0.3, 1.0 / 3.0 - 1e-12)
    per, dims, nbins = (True, True, True), (0, 2), (4, 3)
    ref = profileref.table(lam, per, dims, nbins, mass, v)
    edge = profileref.edges(lam, per, dims, nbins)
    assert ref["n_edge"] == edge["n_edge"] == 3
    want = np.zeros(12, dtype=int)
    for r in (1 * 3 + 0, 2 * 3 + 0, 0 * 3 + 1, 0 * 3 + 2, 3 * 3 + 0, 3 * 3 + 1, 0 * 3 + 0, 0 * 3 + 1):     # (x 1|2, z 0), (x 0, z 1|2), (x 3|0, z 0|1)
        want[r] += 1
    assert edge["may"].tolist() == want.tolist() and edge["placed"].sum() == 3 and np.all(edge["placed"] <= edge["may"])
    with pytest.raises(AssertionError):
        profileref.check_sums(ref["count"], ref["sums"], ref["exponents"], ref)
    worst, n_edge = profileref.check_sums_with_edges(ref["count"], ref["sums"], ref["exponents"], ref, edge)
    assert n_edge == 3 and 0.0 < worst <= 0.5
    other = profileref.table(np.vstack([[0.5 + 1e-12, 0.3, 0.2], lam[1:]]), per, dims, nbins, mass, v, exponents=ref["exponents"])
    assert not np.array_equal(other["count"], ref["count"])
    profileref.check_sums_with_edges(other["count"], other["sums"], ref["exponents"], ref, edge)
    moved = ref["count"].copy()
    moved[5] -= 1
    moved[8] += 1                                     # rows (1, 2) and (2, 2): no planted atom can fall there
    assert edge["may"][5] == edge["may"][8] == 0
    with pytest.raises(AssertionError):
        profileref.check_sums_with_edges(moved, ref["sums"], ref["exponents"], ref, edge)
    off = ref["sums"].copy()
    off[5, 4] += 4 * ref["count"][5]
    with pytest.raises(AssertionError):
        profileref.check_sums_with_edges(ref["count"], off, ref["exponents"], ref, edge)
    lam2 = _atoms(seed=11)[0]
    ref2, edge2 = profileref.table(lam2, per, dims, nbins, mass, v), profileref.edges(lam2, per, dims, nbins)
    assert edge2["n_edge"] == 0 and not edge2["may"].any()
    assert profileref.check_sums_with_edges(ref2["count"], ref2["sums"], ref2["exponents"], ref2, edge2)[0] == \
        profileref.check_sums(ref2["count"], ref2["sums"], ref2["exponents"], ref2)


@pytest.mark.parametrize("com", [False, True])
def test_profile_normalise_against_the_reference(com):
    lam, mass, v = _atoms(seed=9)
    nbins = (3, 9)                                     # 27 rows of 700 atoms over 1.6 box lengths: some stay empty
    ref = profileref.table(lam, (False, False, False), (0, 2), nbins, mass, v + np.array([3.0, -2.0, 1.0]))
    ref["count"][5], ref["sums"][5] = 0, 0
    args = (ref["count"], ref["sums"], ref["exponents"], nbins, 1234.5, S.BOLTZ, S.MVV2E, 1.0 / 0.602214129, com)
    got, want = resident.profile_normalise(*args), profileref.normalise(*args)
    assert got.shape == want.shape == (27, 9)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
    assert np.all(got[5, 2:] == 0.0) and got[5, 0] == (0 + 0.5) / 3 and got[5, 1] == (5 + 0.5) / 9
    full = ref["count"] > 0
    # density/mass x vcm summed over the bins is the momentum of the atoms in them, whatever the bins are
    px = (mass * (v[:, 0] + 3.0))[profileref.bins(lam, (False,) * 3, (0, 2), nbins)[0] != 5].sum()
    assert np.all(got[full, 5] > 0.0) and np.isclose((got[:, 4] * got[:, 6]).sum() * (1234.5 / 27) * 0.602214129, px, rtol=1e-12)
    assert np.isclose(got[:, 2].sum(), ref["count"].sum()) and np.isclose(got[:, 3].sum() * 1234.5 / 27, ref["count"].sum())


def test_two_halves_carry_an_int64_through_a_sum_of_doubles():
    rng = np.random.default_rng(2)
    world = 8
    q = rng.integers(-2 ** 58, 2 ** 58, size=(world, 300), dtype=np.int64)      # 8 of them stay below 2^61
    q[:, 0] = [2 ** 58 - 1, -2 ** 58, 1, -1, 0, 2 ** 31, -2 ** 31, 2 ** 31 - 1]
    q[:, 1] = -1
    halves = [resident.profile_split(r) for r in q]
    assert all(h.dtype == np.float64 and l.dtype == np.float64 for h, l in halves)
    assert all(np.all(np.abs(h) <= 2.0 ** 27) and np.all((0 <= l) & (l < 2.0 ** 31)) for h, l in halves)
    hi, lo = sum(h for h, _ in halves), sum(l for _, l in halves)                # what a transport's sum of doubles returns
    total = resident.profile_join(np.rint(hi), np.rint(lo))
    assert total.dtype == np.int64 and np.array_equal(total, q.sum(axis=0))
    assert total[1] == -world
    naive = np.rint(q.astype(np.float64).sum(axis=0)).astype(np.int64)           # not vacuous: whole doubles lose the low bits
    assert not np.array_equal(naive, total)


def test_the_exponent_rule():
    """N (r 2^e + 1/2) < 2^62 in exact arithmetic for r from 1e-300 to 1e300 and N from 1 to 2^40, with the headroom used to
    within a factor 4; the library's copy and the reference's agree everywhere"""
    assert capi.profile_exponent(0.0, 1000) == 0 and profileref.exponent(0.0, 1000) == 0
    rs = [10.0 ** p for p in range(-300, 301, 12)] + [1.0, 2.0, 0.5, 2.0 ** -1022, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 3.9999, 4.0,
                                                        1.7e308]
    ns = [1, 2, 3, 4, 5, 864, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 3_980_000, 2 ** 31, 2 ** 40 - 1, 2 ** 40]
    for r in rs:
        for n in ns:
            e = capi.profile_exponent(r, n)
            assert e == profileref.exponent(r, n), (r, n)
            scaled = Fraction(r) * Fraction(2) ** e
            assert n * (scaled + Fraction(1, 2)) < 2 ** 62, (r, n, e)
            assert max(n, 2) * scaled >= 2 ** 59, (r, n, e)
            assert abs(e) < 2000
