"""CPU: the masked host loops of the group tests (tests/groupref.py) pinned on their own.  With an all-true mask they
reproduce nhcref.run_nvt and langevinref.run_langevin bit for bit -- the masked reference IS the reference --, with a
real mask the held atoms never move, the thermostats act on their groups alone, and the exported names of the group
calls are listed where the bindings look for them."""
import numpy as np

from lammps_plugins_amd.host import capi, system as S
import groupref
import langevinref
import nhcref

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


def test_all_true_mask_reproduces_run_nvt_bit_for_bit():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    nhc = lambda: nhcref.NHC(300.0, 450.0, 0.05, 3 * len(m) - 3, 0.002, tchain=3, boltz=BOLTZ, mvv2e=MVV2E)   # noqa: E731
    xa, va = nhcref.run_nvt(x.copy(), v.copy(), m, _force, nhc(), 0, 200, FTM2V)
    xb, vb = groupref.run_nvt(x.copy(), v.copy(), m, _force, nhc(), 0, 200, FTM2V, np.ones(len(m), dtype=bool))
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert not np.array_equal(xa, x)


def test_all_true_mask_reproduces_run_langevin_bit_for_bit():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    lgv = lambda: langevinref.Langevin(300.0, 900.0, 0.05, 9911, mass, 0.002, FTM2V, boltz=BOLTZ, mvv2e=MVV2E,   # noqa: E731
                                       ratio={1: 2.0, 2: 0.5}, zero=True, tally=True)
    a, b = lgv(), lgv()
    every = np.ones(len(m), dtype=bool)
    xa, va = langevinref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, a, 0, 200, FTM2V)
    xb, vb = groupref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, b, 0, 200, FTM2V, every, every)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert a.scalar() == b.scalar() != 0.0


def test_a_real_mask_holds_the_rest_and_thermostats_the_groups_alone():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g = (tag % 5 != 0) & (tag > 100)
    l = g & (tag % 2 == 0)
    # NVT on the group: held atoms bitwise, the chain's temperature is the group's
    nhc = nhcref.NHC(300.0, 300.0, 0.05, 3 * int(g.sum()) - 3, 0.002, boltz=BOLTZ, mvv2e=MVV2E)
    xb, vb = groupref.run_nvt(x.copy(), v.copy(), m, _force, nhc, 0, 50, FTM2V, g)
    assert np.array_equal(xb[~g], x[~g]) and np.array_equal(vb[~g], v[~g])
    assert not np.array_equal(xb[g], x[g])
    assert nhc.T == nhc.temperature(vb[g], m[g])
    # Langevin on a sub-group: the mean of `zero` is the sub-group's, the other group atoms follow plain Verlet
    lgv = langevinref.Langevin(300.0, 300.0, 0.05, 9911, mass, 0.002, FTM2V, boltz=BOLTZ, mvv2e=MVV2E, zero=True, tally=True)
    fl = groupref.lgv_force(lgv, 7, tag, type_, v, l)
    assert np.all(fl[~l] == 0.0) and np.all(fl[l] != 0.0)
    fran = lgv.random(7, tag[l], type_[l])
    want = lgv.g1[type_[l]][:, None] * v[l] + fran - fran.sum(axis=0) / int(l.sum())
    assert np.array_equal(fl[l], want)
    xc, vc = groupref.run_langevin(x.copy(), v.copy(), m, tag, type_, _force, lgv, 0, 50, FTM2V, g, l)
    assert np.array_equal(xc[~g], x[~g]) and np.array_equal(vc[~g], v[~g])
    plain = g & ~l
    xs, vs = x.copy(), v.copy()
    dtf = 0.5 * 0.002 * FTM2V
    f = _force(xs)[0]
    for _ in range(50):
        vs[plain] += dtf * f[plain] / m[plain][:, None]
        xs[plain] += 0.002 * vs[plain]
        f = _force(xs)[0]
        vs[plain] += dtf * f[plain] / m[plain][:, None]
    assert np.array_equal(xc[plain], xs[plain]) and np.array_equal(vc[plain], vs[plain])
    assert lgv.scalar() != 0.0


def test_the_test_masks_meet_their_conditions():
    for s in (S.replicate(S.rebomos_bulk_cell(), (2, 2, 1)), S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)):
        by_tag, g, lg = groupref.masks(s)
        groupref.check_masks(s, g, lg)
        assert np.all(by_tag[s.tag] & groupref.ALL_BIT)
        assert np.array_equal((by_tag[s.tag] & groupref.INTEGRATE_BIT) != 0, g)
        assert np.array_equal((by_tag[s.tag] & groupref.LANGEVIN_BIT) != 0, lg)


def test_group_calls_are_listed_for_the_bindings():
    for name in ("mdp_md_set_mask", "mdp_hnve_set_mask", "mdp_integrate_group", "mdp_langevin_group"):
        assert name in capi.EXPORTS
    for method in ("md_set_mask", "hnve_set_mask", "integrate_group", "langevin_group"):
        assert callable(getattr(capi.Context, method))
