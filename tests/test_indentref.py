"""CPU: the host reference of the indenters (tests/indentref.py).  The force is minus the gradient of the energy for every
shape and side; the force on the indenter is minus the sum of the atoms'; an atom across a periodic face of the tilted MoS2
cell feels the image nearest the centre; `vel` moves the centre as vdisplace would and starts again at `first`; a static
indenter in the host loop conserves KE + E_pair + E_indenter as well as the plain loop conserves KE + E_pair; the new calls
are exported."""
import numpy as np
import pytest

from conftest import POT_AEAM
from lammps_plugins_amd.host import capi, resident, system as S
import bathsref
import indentref
import mdref

RNG = np.random.default_rng(12)


def _mos2():
    return S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))


SHAPES = [dict(shape="sphere", side="out"), dict(shape="sphere", side="in"),
          dict(shape="cylinder", side="out", dim=0), dict(shape="cylinder", side="in", dim=1), dict(shape="cylinder", side="out", dim=2),
          dict(shape="plane", side="lo", dim=2), dict(shape="plane", side="hi", dim=0), dict(shape="plane", side="hi", dim=1)]


def _indenter(q, box):
    """the shape q in the middle of the box, with a radius that leaves atoms on both sides of its surface"""
    c = box.lamda2x(np.array([[0.52, 0.47, 0.55]]))[0]
    return dict(q, k=3.7, r=5.0 if q["side"] == "out" else 7.0, c=c)


@pytest.mark.parametrize("q", SHAPES, ids=lambda q: f"{q['shape']}-{q['side']}-{q.get('dim', 0)}")
def test_the_force_is_minus_the_gradient_and_the_indenter_feels_minus_the_sum(q):
    s = _mos2()
    ind = _indenter(q, s.box)
    x = S.wrap(s.box, s.x)
    f = np.zeros_like(x)
    st = indentref.post_force([ind], 0, 0, 0.001, s.box, x, f)[0]
    assert 20 < st["contacts"] < s.n - 20
    assert np.abs(st["force"] + f.sum(axis=0)).max() <= 1e-12 * np.abs(f).sum()
    touched = np.flatnonzero(np.abs(f).sum(axis=1) > 0.0)
    assert len(touched) == st["contacts"]

    def energy(i, xi):
        return float(indentref.terms(ind, ind["c"], s.box, xi[None])[1][0])
    h = 1e-5
    for i in RNG.choice(touched, 12, replace=False):
        # central differences of the atom's own cubic term: off by K h^2 / 3 (1.2e-10) and by the rounding of its energy
        # e_i, twice half an ulp over 2 h
        tol = 1e-9 + 4.0 * np.finfo(float).eps * energy(i, x[i]) / h
        for c in range(3):
            xp, xm = x[i].copy(), x[i].copy()
            xp[c] += h
            xm[c] -= h
            assert abs(-(energy(i, xp) - energy(i, xm)) / (2.0 * h) - f[i, c]) < tol, (i, c)
    # an untouched atom feels nothing, and the energy is that of the touching atoms alone
    dr = indentref.depth(ind, ind["c"], s.box, x)[0]
    assert st["energy"] == pytest.approx(float((-(ind["k"] / 3.0) * dr[dr < 0.0] ** 3).sum()), rel=1e-13)
    assert st["energy"] > 0.0


def test_an_atom_across_a_periodic_face_of_the_tilted_cell_feels_the_nearest_image():
    s = _mos2()
    box = s.box
    assert box.tilt[0] != 0.0                                # xy: the cell is tilted
    ind = dict(shape="sphere", side="out", k=2.0, r=3.0, c=box.lamda2x(np.array([[0.02, 0.97, 0.03]]))[0])
    # an atom 1 A from the surface as the crow flies through the faces: on the far side of all three of them
    u = np.array([0.3, -0.5, 0.4])
    u /= np.linalg.norm(u)
    near = ind["c"] + 2.0 * u
    far = near + box.h @ np.array([1.0, -1.0, 1.0])
    for shift in (np.zeros(3), box.h @ np.array([1.0, -1.0, 1.0]), box.h @ np.array([0.0, -1.0, 0.0]), box.h @ np.array([-1.0, 0.0, 1.0])):
        f = np.zeros((1, 3))
        st = indentref.post_force([ind], 0, 0, 0.001, box, (near + shift)[None], f)[0]
        assert st["contacts"] == 1
        assert np.allclose(f[0], 2.0 * 1.0 * u, rtol=0.0, atol=1e-12), shift
    assert np.linalg.norm(far - ind["c"]) > 10.0
    # a wrap in y carries xy into x: without it the atom would sit |xy| further along x and out of reach
    d = indentref.minimum_image(box, (near + box.h @ np.array([0.0, 1.0, 0.0]) - ind["c"])[None])[0]
    assert np.allclose(d, 2.0 * u, atol=1e-12)
    # one wrap per dimension, as LAMMPS: two boxes away is not brought home
    d2 = indentref.minimum_image(box, (near + box.h @ np.array([2.0, 0.0, 0.0]) - ind["c"])[None])[0]
    assert np.allclose(d2, 2.0 * u + box.h @ np.array([1.0, 0.0, 0.0]), atol=1e-12)
    # a dimension that is not periodic is not wrapped
    d3 = indentref.minimum_image(box, (near + box.h @ np.array([0.0, 0.0, 1.0]) - ind["c"])[None], periodic=(True, True, False))[0]
    assert np.allclose(d3, 2.0 * u + box.h @ np.array([0.0, 0.0, 1.0]), atol=1e-12)


def test_a_cylinder_ignores_its_axis_and_a_point_on_the_axis_gets_no_force_but_its_energy():
    s = _mos2()
    ind = dict(shape="cylinder", side="out", dim=2, k=1.5, r=2.0, c=np.array([5.0, 6.0, 123.0]))
    x = np.array([[6.0, 6.0, 1.0], [6.0, 6.0, 9.0], [5.0, 6.0, 3.0]])
    f = np.zeros_like(x)
    st = indentref.post_force([ind], 0, 0, 0.001, s.box, x, f)[0]
    assert st["contacts"] == 3
    assert np.array_equal(f[0], f[1]) and np.allclose(f[0], [1.5, 0.0, 0.0])
    assert not f[2].any()                                   # r = 0: LAMMPS divides by zero there; no force here
    assert st["energy"] == pytest.approx(2 * 1.5 / 3.0 + 1.5 / 3.0 * 8.0)
    with np.errstate(all="raise"):                           # ... and no warning on the way
        indentref.post_force([ind], 0, 0, 0.001, s.box, x)


def test_vel_moves_the_centre_as_vdisplace_and_starts_again_at_first():
    ind = dict(shape="sphere", k=1.0, r=1.0, c=(1.0, 2.0, 3.0), vel=(0.5, 0.0, -2.0))
    dt = 0.002
    assert np.array_equal(indentref.centre(ind, 7, 7, dt), [1.0, 2.0, 3.0])
    assert np.allclose(indentref.centre(ind, 17, 7, dt), [1.0 + 0.5 * 10 * dt, 2.0, 3.0 - 2.0 * 10 * dt], rtol=0, atol=1e-15)
    assert np.array_equal(indentref.centre(ind, 1010, 1000, dt), indentref.centre(ind, 17, 7, dt))
    assert np.array_equal(indentref.centre(dict(ind, vel=(0, 0, 0)), 99, 7, dt), [1.0, 2.0, 3.0])
    # in the loop: harmonic wells, one atom under a plane that comes down on it
    m = np.array([10.0])
    seen = []
    indentref.run(np.zeros((1, 3)), np.zeros((1, 3)), m, lambda x: (-x, 0.0),
                  [dict(shape="plane", side="hi", dim=2, k=1.0, c=(0.0, 0.0, 0.05), vel=(0.0, 0.0, -10.0))], 5, 25, dt, S.FTM2V, [True],
                  S.Box(np.zeros(3), np.full(3, 10.0), np.zeros(3)), on_step=lambda n, x, v, pe, st: seen.append((n, st[0])))
    assert [n for n, _ in seen] == list(range(5, 26))
    assert seen[0][1]["centre"][2] == 0.05 and seen[0][1]["contacts"] == 0
    assert seen[-1][1]["centre"][2] == pytest.approx(0.05 - 10.0 * 20 * dt)
    assert seen[-1][1]["contacts"] == 1 and seen[-1][1]["force"][2] > 0.0    # the atom pushes the plane back up


def test_a_static_indenter_conserves_energy_as_well_as_the_plain_loop(oracle):
    """KE + E_pair + E_indenter over 200 steps of 1 fs on the AEAM cell of the GPU tests, a sphere of R = 2.3 A on an
    octahedral site (its six neighbours stand at a / 2 = 2.02 A) inside the integrate group.  The bound is ten times the
    drift of KE + E_pair in the same loop without the indenter -- velocity Verlet's own error at this step -- not a number
    taken from the run with it"""
    af = capi.AeamFile(POT_AEAM)
    s = S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)
    s.mass[1:3] = af.mass[:2]
    v0 = S.gaussian_velocities(s, 300.0, seed=93)
    _, g, _ = bathsref.masks(s)
    T = oracle.aeam_pot(POT_AEAM)
    make = lambda sy: mdref.AeamCPU(oracle, T, sy, skin=1.0)     # noqa: E731
    every = set(range(1, 201))
    ind = dict(shape="sphere", side="out", k=5.0, r=2.3, c=np.array([3.5, 3.5, 3.5]) * 4.045)

    def spread(inds):
        out, worst = indentref.host_indent(make, s, v0, 200, every, 25, g, inds, energies=True)
        e = np.array([out[n][3][0] + out[n][3][1] + sum(q["energy"] for q in out[n][1]) for n in sorted(out)])
        return float(e.max() - e.min()), out, worst
    plain, _, _ = spread([])
    with_it, out, worst = spread([ind])
    ei = np.array([out[n][1][0]["energy"] for n in sorted(out)])
    print(f"KE + E_pair spread {plain:.3e} eV plain; with the sphere {with_it:.3e} eV, while E_indenter spans {ei.max() - ei.min():.3e} eV")
    assert all(out[n][1][0]["contacts"] >= 6 for n in sorted(out))
    assert ei.max() - ei.min() > 10.0 * plain                # the indenter's energy is a term that matters
    assert with_it < 10.0 * plain, (with_it, plain)


def test_the_four_calls_are_exported_and_the_domain_has_its_methods():
    assert {"mdp_indent_setup", "mdp_indent_run", "mdp_indent_state", "mdp_indent_off"} <= set(capi.EXPORTS)
    L = capi.lib()
    for name in ("mdp_indent_setup", "mdp_indent_run", "mdp_indent_state", "mdp_indent_off"):
        assert hasattr(L, name)
    for name in ("indent", "indent_run", "indent_state", "indent_off"):
        assert callable(getattr(resident.DeviceDomain, name))
    import ctypes
    assert ctypes.sizeof(capi.IndentConfig) == 3 * 4 + 4 + 8 * 8    # three ints, padding, k, c[3], r, vel[3]
    assert (capi.INDENT_MAX, capi.INDENT_STATE_LEN) == (4, 10)
