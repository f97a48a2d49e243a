"""CPU: the NumPy Nose-Hoover chain (tests/nhcref.py) that the `fix nvt/mdp` GPU tests use as their host reference, pinned
on 1 000 independent 3-D harmonic oscillators with analytic forces (reduced units: kB = mvv2e = ftm2v = 1): the
extended energy KE + PE + thermostat energy is conserved, the time-averaged temperature is the target, a ramp ends at
Tstop."""
import numpy as np
import pytest

import nhcref


def _oscillators(tchain, t_start, t_stop, steps=20000, dt=0.005, tdamp=0.5, t_init=1.0, tloop=1, drag=0.0):
    rng = np.random.default_rng(7)
    n = 1000
    m = rng.uniform(0.5, 2.0, n)
    k = rng.uniform(0.5, 2.0, n)
    x = rng.normal(size=(n, 3)) * np.sqrt(t_init / k)[:, None]
    v = rng.normal(size=(n, 3)) * np.sqrt(t_init / m)[:, None]

    def force(x):
        return -k[:, None] * x, 0.5 * float(np.sum(k[:, None] * x * x))

    nhc = nhcref.NHC(t_start, t_stop, tdamp, 3 * n - 3, dt, tchain=tchain, tloop=tloop, drag=drag, boltz=1.0, mvv2e=1.0)
    e, t = [], []

    def on_step(step, x, v, pe):
        e.append(0.5 * float(np.sum(m * np.sum(v * v, axis=1))) + pe + nhc.energy())
        t.append(nhc.T)

    nhcref.run_nvt(x, v, m, force, nhc, 0, steps, 1.0, on_step)
    return np.array(e), np.array(t), nhc


@pytest.mark.parametrize("tchain", [1, 3])
def test_extended_energy_is_conserved_and_temperature_is_the_target(tchain):
    e, t, _ = _oscillators(tchain, 1.0, 1.0)
    assert np.abs(e - e[0]).max() / abs(e[0]) < 1e-5
    assert abs(t[len(t) // 2:].mean() - 1.0) < 0.02


def test_ramp_ends_at_tstop():
    _, t, nhc = _oscillators(3, 0.5, 1.5, t_init=0.5)
    assert nhc.tt == 1.5
    assert abs(t[-200:].mean() - 1.5) < 0.05 * 1.5


def test_drag_and_sub_steps_damp_the_chain():
    """drag takes energy out of the chain: the extended energy is no longer conserved, the temperature still follows"""
    e, t, nhc = _oscillators(4, 1.0, 1.0, steps=4000, t_init=0.3, tloop=2, drag=0.2)
    assert abs(t[len(t) // 2:].mean() - 1.0) < 0.03
    assert len(nhc.eta) == 4 and nhc.eta_dot[4] == 0.0
