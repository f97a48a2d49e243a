"""CPU: the host reference of the heat sources (tests/heatref.py) pinned on harmonic wells, the oscillators of
tests/test_bathsref.py.  One application changes the group's kinetic energy about its centre of mass by eflux nevery dt and
keeps its momentum; eflux = 0 is the plain group loop bit for bit; nevery = 3 applies on steps 3, 6, ... only; two sources
do not depend on their order; a sink that would take more than the group holds raises; the new calls are exported."""
import numpy as np
import pytest

from lammps_plugins_amd.host import capi, resident
import heatref

MVV2E = 1.0364269e-4
FTM2V = 1.0 / MVV2E
K = 1.0     # eV / A^2: harmonic wells
DT = 0.002


def _oscillators(n=300, seed=3):
    rng = np.random.default_rng(seed)
    mass = np.array([0.0, 50.0, 95.94])
    type_ = rng.integers(1, 3, n)
    return mass, type_, np.arange(1, n + 1), rng.normal(0.0, 0.05, (n, 3)), rng.normal(0.0, 1.5, (n, 3))


def _force(x):
    return -K * x, 0.5 * K * float(np.sum(x * x))


def _groups(tag):
    g = tag % 5 != 0
    return g, g & (tag % 4 == 0), g & (tag % 4 == 1) & (tag < 200)


def _plain(x, v, m, g, nsteps):
    dtf = 0.5 * DT * FTM2V
    f = _force(x)[0]
    for _ in range(nsteps):
        v[g] += dtf * f[g] / m[g][:, None]
        x[g] += DT * v[g]
        f = _force(x)[0]
        v[g] += dtf * f[g] / m[g][:, None]
    return x, v


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("nevery", [1, 3])
def test_one_application_adds_eflux_nevery_dt_and_keeps_the_momentum(sign, nevery):
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g, a, b = _groups(tag)
    v[a] += np.array([0.5, -0.3, 0.2])
    ke0 = heatref.kecm(v, m, a, FTM2V, MVV2E)
    eflux = sign * 1e-3 * ke0 * MVV2E / DT               # (kecm is in ke ftm2v units: times mvv2e -> energy)
    p0 = (m[a][:, None] * v[a]).sum(axis=0)
    before = v.copy()
    scale, vcm, den = heatref.apply(v, m, a, eflux, nevery, DT, FTM2V, MVV2E)
    assert den == ke0 and (scale > 1.0) == (sign > 0.0)
    gained = (heatref.kecm(v, m, a, FTM2V, MVV2E) - ke0) * MVV2E
    assert gained == pytest.approx(eflux * nevery * DT, rel=1e-12)
    p1 = (m[a][:, None] * v[a]).sum(axis=0)
    assert np.abs(p1 - p0).max() <= 1e-12 * float(np.sum(m[a][:, None] * np.abs(v[a])))
    assert np.array_equal(v[~a], before[~a]) and not np.array_equal(v[a], before[a])


def test_no_flux_is_the_plain_group_loop_bit_for_bit():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g, a, b = _groups(tag)
    src = [dict(group=a, eflux=0.0, nevery=1), dict(group=b, eflux=0.0, nevery=2)]
    xa, va = heatref.run(x.copy(), v.copy(), m, _force, src, 0, 200, DT, FTM2V, MVV2E, g)
    xb, vb = _plain(x.copy(), v.copy(), m, g, 200)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert np.array_equal(xa[~g], x[~g]) and np.array_equal(va[~g], v[~g])


def test_nevery_three_applies_on_steps_3_6_only_and_the_energy_adds_up():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g, a, b = _groups(tag)
    fa = 1e-3 * heatref.kecm(v, m, a, FTM2V, MVV2E) * MVV2E / DT
    fb = -1e-3 * heatref.kecm(v, m, b, FTM2V, MVV2E) * MVV2E / DT
    for nevery in (1, 3):
        src = [dict(group=a, eflux=fa, nevery=nevery), dict(group=b, eflux=fb, nevery=nevery)]
        seen, scales, energy = [], [], []

        def on_step(n, xs, vs, pe, applied):
            if applied:
                seen.append(n)
                assert sorted(applied) == [0, 1]
                scales.extend(r[0] for r in applied.values())
            energy.append(pe + 0.5 * MVV2E * float(np.sum(m[:, None] * vs * vs)))
        x0, v0 = x.copy(), v.copy()
        e0 = _force(x0)[1] + 0.5 * MVV2E * float(np.sum(m[:, None] * v0 * v0))
        heatref.run(x0, v0, m, _force, src, 0, 200, DT, FTM2V, MVV2E, g, on_step)
        assert seen == [n for n in range(1, 201) if n % nevery == 0]
        assert 0.5 < min(scales) ** 2 < 1.0 < max(scales) ** 2 < 1.5       # (the source heats, the sink cools, neither runs dry)
        # the energy put in is (fa + fb) dt per step of the run, to the integrator's own fluctuation (some 1e-4 eV here)
        assert energy[-1] - e0 == pytest.approx((fa + fb) * DT * nevery * (200 // nevery), abs=1e-3)
        assert abs(fa + fb) * DT * 200 > 1e-2


def test_two_sources_do_not_depend_on_their_order():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g, a, b = _groups(tag)
    src = [dict(group=a, eflux=2.0, nevery=1), dict(group=b, eflux=-1.0, nevery=3)]
    xa, va = heatref.run(x.copy(), v.copy(), m, _force, src, 0, 200, DT, FTM2V, MVV2E, g)
    xb, vb = heatref.run(x.copy(), v.copy(), m, _force, src[::-1], 0, 200, DT, FTM2V, MVV2E, g)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    xc, vc = _plain(x.copy(), v.copy(), m, g, 200)
    assert not np.array_equal(va[a], vc[a]) and not np.array_equal(va[b], vc[b])
    free = g & ~(a | b)
    assert free.sum() > 20 and np.array_equal(xa[free], xc[free]) and np.array_equal(va[free], vc[free])


def test_a_sink_that_takes_more_than_the_group_holds_raises():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    g, a, b = _groups(tag)
    ke0 = heatref.kecm(v, m, a, FTM2V, MVV2E) * MVV2E
    before = v.copy()
    with pytest.raises(heatref.HeatError, match="kinetic energy went negative"):
        heatref.apply(v, m, a, -2.0 * ke0 / DT, 1, DT, FTM2V, MVV2E)
    assert np.array_equal(v, before)
    heatref.apply(v, m, a, -0.5 * ke0 / DT, 1, DT, FTM2V, MVV2E)


def test_the_heat_calls_are_exported():
    assert {"mdp_heat_setup", "mdp_heat_run", "mdp_heat_state", "mdp_heat_off"} <= set(capi.EXPORTS)
    assert capi.HEAT_MAXSRC == 4 and capi.HEAT_STATE_LEN == 8
    for name in ("heat_setup", "heat_run", "heat_state", "heat_off"):
        assert hasattr(capi.Context, name)
    for name in ("heat", "heat_state", "heat_off"):
        assert hasattr(resident.DeviceDomain, name)
