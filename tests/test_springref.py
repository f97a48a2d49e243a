"""CPU: the host reference of the tether springs (tests/springref.py) against closed forms.  Two atoms of unequal mass; a
rest length beyond the distance pushes and gives a negative ftotal[3]; a tether point exactly on the centre of mass; NULL
dimensions; the forces on the group sum to ftotal; the image flags enter the centre of mass; `vel` moves the tether point
and starts again at `first`; a free rigid pair on a spring conserves E + KE; the new calls are exported."""
import math

import numpy as np
import pytest

from lammps_plugins_amd.host import capi, resident, system as S
import springref

BOX = S.Box(np.zeros(3), np.array([20.0, 30.0, 40.0]), np.array([3.0, -2.0, 5.0]))
M2 = np.array([3.0, 1.0])
X2 = np.array([[1.0, 2.0, 3.0], [5.0, 2.0, 3.0]])          # xcm = (2, 2, 3)
NOIMG = np.zeros((2, 3), dtype=np.int64)


def _one(sp, x=X2, m=M2, img=NOIMG, f=None, n=0, first=0):
    return springref.post_force([sp], n, first, 0.001, BOX, x, img, m, f)[0]


def test_two_atoms_of_unequal_mass():
    f = np.zeros((2, 3))
    st = _one(dict(k=2.0, r0=1.0, c=(2.0, 6.0, 3.0)), f=f)
    assert st["mass"] == 4.0 and st["atoms"] == 2 and np.array_equal(st["xcm"], [2.0, 2.0, 3.0])
    # d = (0, -4, 0), r = 4, dr = 3, F = K d dr / r = (0, -6, 0): the group is pulled towards the tether point by 6
    assert st["dr"] == 3.0 and st["energy"] == 9.0
    assert np.array_equal(st["ftotal"], [0.0, 6.0, 0.0, 6.0])
    assert np.array_equal(f, [[0.0, 4.5, 0.0], [0.0, 1.5, 0.0]])          # by mass: 3/4 and 1/4 of it


def test_a_rest_length_beyond_the_distance_pushes_and_ftotal_3_is_negative():
    f = np.zeros((2, 3))
    st = _one(dict(k=2.0, r0=6.5, c=(2.0, 6.0, 3.0)), f=f)
    assert st["dr"] == -2.5 and st["energy"] == 0.5 * 2.0 * 2.5 * 2.5
    assert np.array_equal(st["ftotal"], [0.0, -5.0, 0.0, -5.0])           # away from the tether point
    assert np.array_equal(f.sum(axis=0), st["ftotal"][:3])


def test_a_tether_point_on_the_centre_of_mass():
    k, r0 = 7.0, 1.5
    f = np.zeros((2, 3))
    st = _one(dict(k=k, r0=r0, c=(2.0, 2.0, 3.0)), f=f)
    assert st["dr"] == springref.RMIN - r0
    assert np.abs(f).max() < 1e-9 * k and abs(st["ftotal"][3]) < 1e-9 * k
    assert st["energy"] == pytest.approx(0.5 * k * r0 * r0, rel=1e-9)


@pytest.mark.parametrize("c", [(None, 6.0, None), (5.0, None, 7.0), (None, None, 1.0), (0.5, 6.0, None)])
def test_null_dimensions_take_no_part(c):
    sp = dict(k=2.0, r0=0.5, c=c, vel=(11.0, 12.0, 13.0))
    f = np.zeros((2, 3))
    st = _one(sp, f=f, n=5)
    use = np.array([a is not None for a in c])
    assert not f[:, ~use].any() and not st["ftotal"][:3][~use].any() and not st["tether"][~use].any()
    d = np.where(use, np.array([2.0, 2.0, 3.0]) - st["tether"], 0.0)
    r = math.sqrt(float((d * d).sum()))
    assert np.allclose(st["ftotal"][:3], -2.0 * d * (r - 0.5) / r, rtol=1e-15, atol=0.0)
    assert st["ftotal"][:3][use].all()


def test_the_forces_on_the_group_sum_to_ftotal_and_others_feel_nothing():
    rng = np.random.default_rng(3)
    n = 200
    x = rng.uniform(0.0, 20.0, (n, 3))
    m = rng.uniform(1.0, 100.0, n)
    img = rng.integers(-2, 3, (n, 3))
    group = rng.random(n) < 0.4
    f = np.zeros((n, 3))
    st = springref.post_force([dict(k=3.0, r0=2.0, c=(1.0, None, -4.0), group=group)], 0, 0, 0.001, BOX, x, img, m, f)[0]
    assert st["atoms"] == group.sum() and not f[~group].any()
    assert np.allclose(f.sum(axis=0), st["ftotal"][:3], rtol=0.0, atol=1e-12 * abs(st["ftotal"][3]))
    assert st["ftotal"][3] == pytest.approx(math.sqrt(float((st["ftotal"][:3] ** 2).sum())), rel=1e-15)
    # per atom: proportional to the mass
    assert np.allclose(f[group] / m[group][:, None], -st["fm"][None, :], rtol=1e-14, atol=0.0)
    # a permuted sum and the exact one give the same state to rounding
    for kw in (dict(orders=[rng.permutation(n)]), dict(exact=True)):
        other = springref.post_force([dict(k=3.0, r0=2.0, c=(1.0, None, -4.0), group=group)], 0, 0, 0.001, BOX, x, img, m, **kw)[0]
        assert np.allclose(other["xcm"], st["xcm"], rtol=0.0, atol=1e-12) and other["atoms"] == st["atoms"]


def test_the_image_flags_enter_the_centre_of_mass():
    img = np.array([[1, 0, 0], [-2, 1, 2]])
    st = _one(dict(k=1.0, r0=0.0, c=(0.0, 0.0, 0.0)), img=img)
    h = BOX.h
    xu = X2 + np.array([h @ img[0], h @ img[1]])
    assert np.array_equal(springref.unwrap(BOX, X2, img), xu)
    assert np.allclose(st["xcm"], (3.0 * xu[0] + xu[1]) / 4.0, rtol=1e-15, atol=0.0)
    assert np.abs(st["xcm"] - np.array([2.0, 2.0, 3.0])).min() > 4.0        # boxes away from the wrapped positions


def test_vel_moves_the_tether_point_and_starts_again_at_first():
    sp = dict(k=1.0, r0=0.0, c=(1.0, None, 3.0), vel=(2.0, 5.0, -4.0))
    assert np.array_equal(springref.tether(sp, 7, 7, 0.001), [1.0, 0.0, 3.0])
    assert np.allclose(springref.tether(sp, 107, 7, 0.001), [1.2, 0.0, 2.6], rtol=1e-15)
    big = 2 ** 32 + 7
    assert np.array_equal(springref.tether(sp, big + 100, big, 0.001), springref.tether(sp, 107, 7, 0.001))


def test_a_free_rigid_pair_on_a_spring_conserves_spring_energy_plus_kinetic_energy():
    """no pair forces and equal velocities: f_i = -(F / M) m_i gives both atoms the acceleration of the centre of mass, so the
    pair stays rigid and E + KE is the harmonic oscillator's (R0 = 0), which velocity Verlet conserves to (omega dt)^2 / 4 of it:
    the energy it conserves exactly differs from this one by that fraction of the potential part"""
    m = np.array([27.0, 95.95])
    x = np.array([[1.0, 2.0, 3.0], [2.5, 2.0, 3.5]])
    v = np.tile(np.array([[0.7, -0.4, 0.2]]), (2, 1))
    sp = dict(k=4.0, r0=0.0, c=(3.0, 1.0, 2.0))
    img = np.array([[0, 0, 0], [0, 0, 0]])
    sep0 = x[1] - x[0]
    tot = []

    def on_step(n, x, v, pe, st):
        ke = 0.5 * S.MVV2E * float((m[:, None] * v * v).sum())
        tot.append(st[0]["energy"] + ke)
        assert np.allclose(x[1] - x[0], sep0, rtol=0.0, atol=1e-12)

    springref.run(x, v, m, lambda x: (np.zeros_like(x), 0.0), [sp], 0, 2000, 0.001, S.FTM2V, np.ones(2, dtype=bool), BOX, img, on_step)
    tot = np.array(tot)
    wdt2 = sp["k"] * S.FTM2V / m.sum() * 0.001 ** 2           # (omega dt)^2 of the harmonic oscillator the pair is
    print(f"E + KE over 2000 steps: {tot.min():.9f} .. {tot.max():.9f}, (omega dt)^2 = {wdt2:.2e}")
    assert tot.max() - tot.min() < wdt2 * tot[0], (tot.min(), tot.max())
    assert np.ptp([t for t in tot]) > 0.0                                     # (the spring does act)


def test_the_spring_calls_are_exported_and_wrapped():
    for name in ("mdp_spring_setup", "mdp_spring_run", "mdp_spring_state", "mdp_spring_off"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    for name in ("spring", "spring_run", "spring_state", "spring_off"):
        assert hasattr(resident.DeviceDomain, name)
    import ctypes
    assert ctypes.sizeof(capi.SpringConfig) == 80 and capi.SPRING_STATE_LEN == 16 and capi.SPRING_MAX == 4
