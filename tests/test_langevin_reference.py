"""CPU: the NumPy Langevin thermostat (tests/langevinref.py), the host reference of the `fix langevin/mdp` tests, pinned
on its own: the Philox4x32-10 known-answer vectors (Random123), the map to uniforms, 1 000 harmonic oscillators held at
the target temperature, `zero yes` and the tally's energy balance."""
import numpy as np
import pytest

import langevinref as L

BOLTZ, MVV2E = 8.617343e-5, 1.0364269e-4
FTM2V = 1.0 / MVV2E


def _words(ctr, key):
    return [int(w[0]) for w in L.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)]


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, (0xffffffff, 0xffffffff), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0),
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox_known_answers(ctr, key, want):
    assert _words(ctr, key) == want


def test_uniform_mapping():
    assert L.uniform(0) == 0.5 * 2.0 ** -32
    assert 0.0 < L.uniform(0) and L.uniform(0xFFFFFFFF) < 1.0
    assert L.uniform(0xFFFFFFFF) == 1.0 - 0.5 * 2.0 ** -32
    u = L.noise(7, np.arange(1, 200001), 12345, 0)
    assert u.shape == (200000, 3)
    assert abs(u.mean() - 0.5) < 2e-3 and abs(u.var() - 1.0 / 12.0) < 1e-3
    # the counter words: tag, step (low and high words), phase
    assert not np.array_equal(u, L.noise(7, np.arange(1, 200001), 12345, 1))
    assert not np.array_equal(u, L.noise(7, np.arange(1, 200001), 12345 + (1 << 32), 0))
    assert np.array_equal(u[10:20], L.noise(7, np.arange(11, 21), 12345, 0))


def _oscillators(n=1000, seed=3):
    rng = np.random.default_rng(seed)
    mass = np.array([0.0, 50.0, 95.94])
    type_ = rng.integers(1, 3, n)
    return mass, type_, np.arange(1, n + 1), rng.normal(0.0, 0.05, (n, 3)), np.zeros((n, 3))


def test_harmonic_oscillators_reach_the_target_temperature():
    mass, type_, tag, x, v = _oscillators()
    m = mass[type_]
    k = 1.0                                       # eV / A^2
    target, dt = 300.0, 0.002
    lgv = L.Langevin(target, target, 0.1, 9911, mass, dt, FTM2V, boltz=BOLTZ, mvv2e=MVV2E)
    temps = []

    def on_step(n, x, v, pe):
        if n > 1000:
            temps.append(float(np.sum(m[:, None] * v * v)) * MVV2E / (3 * len(m) * BOLTZ))

    L.run_langevin(x, v, m, tag, type_, lambda x: (-k * x, 0.5 * k * float(np.sum(x * x))), lgv, 0, 5000, FTM2V,
                   on_step)
    assert np.mean(temps) == pytest.approx(target, rel=0.03)


def test_zero_takes_out_the_mean_of_the_random_parts():
    mass, type_, tag, _, _ = _oscillators()
    v = np.zeros((len(tag), 3))
    lgv = L.Langevin(300.0, 300.0, 0.1, 5, mass, 0.001, FTM2V, zero=True)
    fl = lgv.force(10, tag, type_, v)
    assert np.abs(fl.sum(axis=0)).max() < 1e-12 * np.abs(fl).max() * len(tag)
    plain = L.Langevin(300.0, 300.0, 0.1, 5, mass, 0.001, FTM2V).force(10, tag, type_, v)
    assert np.abs(plain.sum(axis=0)).max() > 1e-3 * np.abs(plain).max()


def _drag_run(dt, t_end=2.0):
    """T = 0: drag only; returns the drift of etotal and of etotal + the thermostat energy"""
    mass, type_, tag, x, _ = _oscillators(200)
    v = np.random.default_rng(4).normal(0.0, 5.0, x.shape)
    m = mass[type_]
    k = 1.0
    lgv = L.Langevin(0.0, 0.0, 0.5, 77, mass, dt, FTM2V, boltz=BOLTZ, mvv2e=MVV2E, tally=True)
    ke = lambda v: 0.5 * MVV2E * float(np.sum(m[:, None] * v * v))
    e0 = ke(v) + 0.5 * k * float(np.sum(x * x))
    rows = []
    L.run_langevin(x, v, m, tag, type_, lambda x: (-k * x, 0.5 * k * float(np.sum(x * x))), lgv, 0,
                   int(round(t_end / dt)), FTM2V, lambda n, x, v, pe: rows.append(ke(v) + pe))
    return rows[-1] - e0, rows[-1] + lgv.scalar() - e0


def test_damp_only_energy_balance_is_second_order():
    d1, c1 = _drag_run(0.004)
    d2, c2 = _drag_run(0.002)
    assert abs(d1) > 1.0                          # the drag took most of the energy out
    assert abs(c1) < 1e-3 * abs(d1)               # ... and the tally accounts for it
    assert 3.0 < abs(c1 / c2) < 5.0               # O(dt^2)
