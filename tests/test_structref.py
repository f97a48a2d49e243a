"""CPU: tests/structref.py, the NumPy reference of compute coord/atom/mdp and centro/atom/mdp, on states whose answers are known
from the lattice: the 6 x 6 x 6 fcc cell with a = 4.045 A, perfect, with one atom removed and jittered; the MoS2 cell at 0 K."""
import numpy as np

from lammps_plugins_amd.host import system as S
import structref

PER = (1, 1, 1)
A = 4.045


def _fcc():
    return S.fcc_cell(A, 6)


def vacancy_cell(sigma=0.05, seed=17, gone=431):
    """the 864-atom fcc cell without the atom at row `gone`, every position moved by a normal deviate of sigma A: (x[863][3],
    h, rows of the vacancy's 12 neighbours in x)"""
    s = _fcc()
    d = s.x - s.x[gone]
    d -= np.rint(d / (6 * A)) * (6 * A)
    near = np.nonzero(np.abs((d * d).sum(axis=1) - 0.5 * A * A) < 1e-6)[0]
    assert len(near) == 12
    keep = np.arange(s.n) != gone
    x = s.x[keep] + sigma * np.random.default_rng(seed).standard_normal((s.n - 1, 3))
    return x, s.box.h, near - (near > gone)


def test_the_perfect_lattice():
    """12 neighbours inside 3.5 A for every atom, no edge pair, and a centro-symmetry parameter that is rounding alone"""
    s = _fcc()
    c = structref.coord(s.x, s.type, s.box.h, PER, 3.5, [(1, 1)])
    assert np.all(c["count_sure"][:, 0] == 12) and c["n_edge"] == 0 and not c["edge"].any()
    r = structref.centro(s.x, s.box.h, PER, 12, 3.5)
    assert np.all(r["inside"] == 12) and r["value"].max() < 1e-24 and not r["ambiguous"].any()


def test_columns_and_the_group():
    """one column per type range on a two-type cell: the columns of 1 and 2 add up to that of 1 .. 2; an atom outside the group is
    no centre (all 0) and still a partner"""
    s = S.fcc_cell(A, 4, frac_type2=0.3, seed=5)
    member = np.arange(s.n) % 3 != 0
    c = structref.coord(s.x, s.type, s.box.h, PER, 3.5, [(1, 2), (1, 1), (2, 2)], member)["count_sure"]
    assert np.all(c[member, 0] == 12) and np.all(c[~member] == 0) and np.array_equal(c[:, 0], c[:, 1] + c[:, 2])
    assert c[member, 2].max() > 0 and c[member, 1].max() > 0
    r = structref.centro(s.x, s.box.h, PER, 12, 3.5, member)
    assert np.all(r["value"][~member] == 0.0) and np.all(r["inside"] == 12)


def test_a_vacancy_at_zero_kelvin():
    """the vacancy's 12 neighbours have lost the partner of one of their six opposite pairs: the sixth smallest pair value is
    that of a 90-degree pair, |R_a + R_b|^2 = a^2 / 2 = 8.181 A^2; every other atom is centro-symmetric.  The twelve see their 11
    remaining first neighbours and 6 second neighbours at equal distance for the twelfth place: ambiguous, which is why the
    device tests are thermal."""
    x, h, near = vacancy_cell(sigma=0.0)
    r = structref.centro(x, h, PER, 12, 6.5)
    rest = np.setdiff1d(np.arange(len(x)), near)
    assert r["value"][rest].max() < 2e-28 and set(r["inside"][rest]) == {77, 78}   # (the vacancy is 1 of the 78 of 66 others)
    assert np.all(r["ambiguous"][near]) and r["ambiguous"].sum() == 12
    assert np.allclose(r["value"][near], 0.5 * A * A, rtol=1e-12)


def test_a_vacancy_in_a_jittered_cell(capsys):
    """sigma = 0.05 A: the vacancy's 12 neighbours above 5 A^2, every other atom below 2 A^2, nobody ambiguous; the coordination
    number inside 3.5 A is 11 for the twelve and 12 for the rest"""
    x, h, near = vacancy_cell()
    r = structref.centro(x, h, PER, 12, 6.5)
    rest = np.setdiff1d(np.arange(len(x)), near)
    with capsys.disabled():
        print(f"vacancy's neighbours {r['value'][near].min():.2f} .. {r['value'][near].max():.2f} A^2, the rest at most "
              f"{r['value'][rest].max():.2f} A^2, {int(r['ambiguous'].sum())} ambiguous of {len(x)}")
    assert r["value"][near].min() > 5.0 and r["value"][rest].max() < 2.0 and not r["ambiguous"].any()
    assert set(np.argsort(r["value"])[-12:]) == set(near)
    c = structref.coord(x, np.ones(len(x), dtype=int), h, PER, 3.5, [(1, 1)])
    assert np.all(c["count_sure"][near, 0] == 11) and np.all(c["count_sure"][rest, 0] == 12) and c["n_edge"] == 0


def test_fewer_than_n_inside_gives_zero():
    x, h, near = vacancy_cell()
    r = structref.centro(x, h, PER, 12, 3.5)
    assert np.all(r["inside"][near] == 11) and np.all(r["value"][near] == 0.0) and r["value"].max() > 0.0


def test_an_edge_pair_is_counted_apart():
    """two atoms a cutoff apart to within 1e-12 relative: an edge pair, in neither direction a sure one"""
    x = np.array([[1.0, 1.0, 1.0], [1.0 + 3.0 * (1.0 - 1e-12), 1.0, 1.0], [1.0, 2.5, 1.0]])
    h = np.diag([20.0, 20.0, 20.0])
    c = structref.coord(x, [1, 1, 1], h, PER, 3.0, [(1, 1)])
    assert c["count_sure"][:, 0].tolist() == [1, 0, 1] and c["edge"][:, 0].tolist() == [1, 1, 0] and c["n_edge"] == 2


def test_an_ambiguous_choice_is_flagged():
    """four partners, the second and third at the same distance: N = 2 cannot tell them apart, N = 4 takes them all"""
    x = np.array([[5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [5.0, 6.5, 5.0], [5.0, 5.0, 6.5], [3.0, 5.0, 5.0]])
    h = np.diag([30.0, 30.0, 30.0])
    assert structref.centro(x, h, PER, 2, 2.5)["ambiguous"][0]
    r = structref.centro(x, h, PER, 4, 2.5)
    assert not r["ambiguous"][0] and r["inside"][0] == 4
    # the 2 smallest of the 6 pair values: (1 0 0) + (-2 0 0) -> 1, and (1.5^2 + 1) twice / (1.5^2 + 1.5^2) / ...
    assert np.isclose(r["value"][0], 1.0 + 3.25)


def test_mos2_at_zero_kelvin():
    """a Mo has 6 S inside 2.8 A and an S has 3 Mo; no Mo-Mo or S-S pair is that close"""
    s = S.rebomos_bulk_cell()
    c = structref.coord(s.x, s.type, s.box.h, PER, 2.8, [(1, 1), (2, 2)])["count_sure"]
    mo, su = s.type == 1, s.type == 2
    assert np.all(c[mo, 1] == 6) and np.all(c[mo, 0] == 0) and np.all(c[su, 0] == 3) and np.all(c[su, 1] == 0)


def test_the_bound_of_the_device_tests():
    """64 eps N Rc Lmax: 2.8e-11 A^2 on the alloy at its limit of 6.5 A"""
    assert abs(structref.centro_bound(12, 6.5, 6 * A) / 2.8e-11 - 1.0) < 0.05
