"""CPU: the several-bath host loops (tests/bathsref.py) pinned on their own.  With one bath they are groupref's bit for
bit; a `zero no` bath split into two baths with the same numbers is the same trajectory bit for bit (the noise is keyed
by tag, so it does not matter which bath draws it) and the two tallies add up to the one; the order of the baths changes
nothing.  The masks of the GPU tests satisfy their conditions on both cells, and the bath calls are exported."""
import numpy as np
import pytest

from lammps_plugins_amd.host import capi, system as S
import bathsref
import groupref
import langevinref

BOLTZ, MVV2E = 8.617343e-5, 1.0364269e-4
FTM2V = 1.0 / MVV2E
K = 1.0   # eV / A^2: harmonic wells


def _oscillators(n=300, seed=3):
    rng = np.random.default_rng(seed)
    mass = np.array([0.0, 50.0, 95.94])
    type_ = rng.integers(1, 3, n)
    return mass, type_, np.arange(1, n + 1), rng.normal(0.0, 0.05, (n, 3)), rng.normal(0.0, 1.5, (n, 3))


def _force(x):
    return -K * x, 0.5 * K * float(np.sum(x * x))


def _lgv(mass, t0=300.0, t1=900.0, damp=0.05, seed=9911, **kw):
    return langevinref.Langevin(t0, t1, damp, seed, mass, 0.002, FTM2V, boltz=BOLTZ, mvv2e=MVV2E, **kw)


def test_one_bath_is_the_group_loop_bit_for_bit():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g = (tag % 5 != 0) & (tag > 100)
    l = g & (tag % 2 == 0)
    a = _lgv(mass, ratio={1: 2.0, 2: 0.5}, zero=True, tally=True)
    b = _lgv(mass, ratio={1: 2.0, 2: 0.5}, zero=True, tally=True)
    xa, va = groupref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, a, 0, 200, FTM2V, g, l)
    xb, vb = bathsref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, [(b, l)], 0, 200, FTM2V, g)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert a.scalar() == b.scalar() != 0.0
    assert not np.array_equal(xa[l], x[l])


def test_a_split_bath_is_the_same_trajectory_and_its_tallies_add_up():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g = (tag % 5 != 0) & (tag > 100)
    l = g & (tag % 3 != 0)
    one = _lgv(mass, tally=True)
    xa, va = bathsref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, [(one, l)], 0, 200, FTM2V, g)
    even, odd = _lgv(mass, tally=True), _lgv(mass, tally=True)
    halves = [(even, l & (tag % 2 == 0)), (odd, l & (tag % 2 == 1))]
    assert halves[0][1].sum() > 20 and halves[1][1].sum() > 20
    xb, vb = bathsref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, halves, 0, 200, FTM2V, g)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert even.scalar() != 0.0 and odd.scalar() != 0.0
    assert even.scalar() + odd.scalar() == pytest.approx(one.scalar(), rel=1e-12)


def test_the_order_of_the_baths_changes_nothing():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g = tag % 5 != 0
    groups = [g & (tag % 4 == 0), g & (tag % 4 == 1) & (tag < 200), g & (tag % 4 == 2)]

    def baths():
        return [(_lgv(mass, 300.0, 900.0, 0.05, 48271, ratio={1: 2.0, 2: 0.5}, zero=True, tally=True), groups[0]),
                (_lgv(mass, 100.0, 100.0, 0.02, 7919, tally=True), groups[1]),
                (_lgv(mass, 600.0, 200.0, 0.1, 48271, zero=True), groups[2])]
    a, b = baths(), baths()
    xa, va = bathsref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, a, 0, 200, FTM2V, g)
    xb, vb = bathsref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, [b[2], b[0], b[1]], 0, 200, FTM2V, g)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert [l.scalar() for l, _ in a] == [l.scalar() for l, _ in b]
    assert a[0][0].scalar() != 0.0 and a[1][0].scalar() != 0.0 and a[2][0].scalar() == 0.0
    # an atom in no bath follows plain Verlet, a held one stays
    free = g & ~(groups[0] | groups[1] | groups[2])
    assert free.sum() > 20
    xs, vs = x.copy(), v.copy()
    dtf = 0.5 * 0.002 * FTM2V
    f = _force(xs)[0]
    for _ in range(200):
        vs[free] += dtf * f[free] / m[free][:, None]
        xs[free] += 0.002 * vs[free]
        f = _force(xs)[0]
        vs[free] += dtf * f[free] / m[free][:, None]
    assert np.array_equal(xa[free], xs[free]) and np.array_equal(va[free], vs[free])
    assert np.array_equal(xa[~g], x[~g]) and np.array_equal(va[~g], v[~g])


def _cells():
    yield "rebomos", S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
    yield "aeam", S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)


def test_the_masks_of_the_gpu_tests_satisfy_their_conditions_on_both_cells():
    for name, s in _cells():
        by_tag, g, baths = bathsref.masks(s)
        bathsref.check_masks(s, g, baths)
        assert np.all(by_tag[s.tag] & bathsref.ALL_BIT)
        assert np.array_equal((by_tag[s.tag] & bathsref.INTEGRATE_BIT) != 0, g)
        assert np.array_equal(g, groupref.masks(s)[1])              # the integrate group of the group tests
        for bit, b in zip(bathsref.BATH_BITS, baths):
            assert np.array_equal((by_tag[s.tag] & bit) != 0, b), name
        by4, g4, baths4 = bathsref.masks4(s)                        # the fourth bath: the three and the group stay as they are
        bathsref.check_masks(s, g4, baths4)
        assert np.array_equal(g4, g) and all(np.array_equal(a, b) for a, b in zip(baths4, baths)) and len(baths4) == 4
        assert np.array_equal(by4[s.tag] & ~32, by_tag[s.tag]) and np.array_equal((by4[s.tag] & 32) != 0, baths4[3]), name
        lam = s.box.x2lamda(S.wrap(s.box, s.x))[:, 0]
        zone = (lam >= 0.5) & (lam < 0.75)                          # ... where lanes of one wave can belong to every bath and to none
        assert all((b & zone).sum() >= 5 for b in baths4) and (g & zone & ~np.logical_or.reduce(baths4)).sum() >= 5, name
    # the check refuses overlapping baths and a bath that leaves the integrate group
    with pytest.raises(AssertionError):
        bathsref.check_masks(s, g, [baths[0], baths[1] | baths[0], baths[2]])
    with pytest.raises(AssertionError):
        bathsref.check_masks(s, g, [baths[0] | (~g & (s.tag % 4 == 0)), baths[1], baths[2]])


def test_the_bath_calls_are_exported():
    assert {"mdp_langevin_baths", "mdp_langevin_tally_bath"} <= set(capi.EXPORTS)
    assert capi.LANGEVIN_MAXBATH == 4
    assert hasattr(capi.Context, "langevin_baths")
