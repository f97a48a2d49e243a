"""No GPU: the host reference of the prescribed group forces (tests/gforceref.py) checked against what LAMMPS' documentation
of fix setforce, fix addforce and fix aveforce promises, and the bounds the device is held to for F_k and E_k
(gforceref.F_TOL, gforceref.E_TOL) derived from the reference's own sensitivity to the order of its sums."""
import math

import numpy as np
import pytest

from lammps_plugins_amd.host import system as S
from refloops import worse
import gforceref
import springref
from test_gpu_gforce_mdp import CASES, EVERY20, NSTEPS, STYLES, XTOL, VTOL, _reference, _case, _group, _ref_slots, _check_reference, A_BIT


def _toy(n=200, seed=3):
    """a small box of atoms with forces, image flags and four overlapping groups"""
    rng = np.random.default_rng(seed)
    box = S.Box(np.zeros(3), np.array([11.0, 12.0, 13.0]), np.array([0.7, -0.4, 0.3]))
    x = box.lamda2x(rng.uniform(0.0, 1.0, (n, 3)))
    img = rng.integers(-2, 3, (n, 3))
    f = rng.normal(0.0, 1.0, (n, 3))
    i = np.arange(n)
    groups = dict(all=None, a=i % 4 == 0, b=i % 4 == 1, ab=i % 4 < 2, half=i < n // 2, none=np.zeros(n, dtype=bool))
    return box, x, img, f, groups


def test_setforce_writes_its_numbers_and_reports_the_force_it_replaced():
    box, x, img, f, G = _toy()
    f0 = f.copy()
    st, = gforceref.post_force([dict(kind="set", f=(0.25, None, -1.0), group=G["a"])], box, x, img, f)
    a = G["a"]
    assert np.all(f[a, 0] == 0.25) and np.all(f[a, 2] == -1.0) and np.array_equal(f[a, 1], f0[a, 1])
    assert np.array_equal(f[~a], f0[~a])
    assert np.allclose(st["ftotal"], f0[a].sum(axis=0), rtol=0.0, atol=1e-12) and st["atoms"] == int(a.sum()) and st["energy"] == 0.0
    assert np.array_equal(st["value"], [0.25, 0.0, -1.0])


def test_after_aveforce_every_atom_of_the_group_holds_the_same_force_and_the_total_is_F_plus_N_f():
    box, x, img, f, G = _toy()
    f0 = f.copy()
    b = G["b"]
    st, = gforceref.post_force([dict(kind="ave", f=(0.5, None, -0.25), group=b)], box, x, img, f)
    n = int(b.sum())
    for d, fd in ((0, 0.5), (2, -0.25)):
        assert np.all(f[b, d] == f[b, d][0])
        assert f[b, d].sum() == pytest.approx(st["ftotal"][d] + n * fd, abs=1e-12)
        assert f[b, d][0] == st["value"][d] == st["ftotal"][d] / n + fd
    assert np.array_equal(f[b, 1], f0[b, 1]) and np.array_equal(f[~b], f0[~b]) and st["value"][1] == 0.0
    assert np.allclose(st["ftotal"], f0[b].sum(axis=0), rtol=0.0, atol=1e-12)
    # a group without atoms: nothing happens
    f1 = f.copy()
    st, = gforceref.post_force([dict(kind="ave", f=(1.0, 1.0, 1.0), group=G["none"])], box, x, img, f)
    assert np.array_equal(f, f1) and st["atoms"] == 0 and not st["ftotal"].any() and not st["value"].any()


def test_addforce_adds_its_numbers_and_its_energy_is_minus_f_dot_the_sum_of_the_unwrapped_positions():
    box, x, img, f, G = _toy()
    f0 = f.copy()
    val = np.array([0.3, -0.2, 0.1])
    st, = gforceref.post_force([dict(kind="add", f=tuple(val), group=G["half"])], box, x, img, f)
    h = G["half"]
    xu = springref.unwrap(box, x, img)
    assert np.array_equal(f[h], f0[h] + val) and np.array_equal(f[~h], f0[~h])
    assert st["energy"] == pytest.approx(-float(val @ xu[h].sum(axis=0)), rel=1e-13)
    assert abs(st["energy"] + float(val @ x[h].sum(axis=0))) > 1.0          # (the wrapped positions give another number)
    assert np.allclose(st["ftotal"], f0[h].sum(axis=0), rtol=0.0, atol=1e-12)
    with pytest.raises(AssertionError):
        gforceref.post_force([dict(kind="add", f=(0.1, None, 0.0), group=None)], box, x, img, f)


def _setforce(f, group, fx, fy, fz):
    """LAMMPS fix setforce on its own, as its documentation states it"""
    tot = f[group].sum(axis=0)
    for d, v in enumerate((fx, fy, fz)):
        if v is not None:
            f[group, d] = v
    return tot


def _aveforce(f, group, fx, fy, fz):
    """LAMMPS fix aveforce on its own, as its documentation states it"""
    tot = f[group].sum(axis=0)
    for d, v in enumerate((fx, fy, fz)):
        if v is not None:
            f[group, d] = tot[d] / group.sum() + v
    return tot


def test_the_walk_gives_set_then_ave_on_shared_atoms_what_two_sequential_fixes_give():
    """a lane walks its atom's slots once; an aveforce is the last of them.  setforce on a and b, addforce on everything,
    then aveforce on b: b's atoms are in three slots"""
    box, x, img, f, G = _toy()
    slots = [dict(kind="set", f=(0.0, None, 0.5), group=G["ab"]), dict(kind="add", f=(0.1, 0.2, -0.3), group=None),
             dict(kind="ave", f=(None, 0.25, -0.125), group=G["b"]), dict(kind="set", f=(None, 0.0, None), group=G["a"])]
    assert not gforceref.shares_with_ave_in_front(slots, len(f))
    # two (here four) fixes, one after the other
    f_seq = f.copy()
    t0 = _setforce(f_seq, G["ab"], 0.0, None, 0.5)
    t1 = f_seq.sum(axis=0)
    f_seq += np.array([0.1, 0.2, -0.3])
    t2 = _aveforce(f_seq, G["b"], None, 0.25, -0.125)
    t3 = _setforce(f_seq, G["a"], None, 0.0, None)
    f_rule = f.copy()
    st_rule = gforceref.post_force(slots, box, x, img, f_rule)
    f_walk, st_walk = gforceref.walk(slots, box, x, img, f.copy())
    assert np.array_equal(f_rule, f_seq) and np.array_equal(f_walk, f_seq)
    for tot, a, b in zip((t0, t1, t2, t3), st_rule, st_walk):
        assert np.allclose(a["ftotal"], tot, rtol=0.0, atol=1e-12) and np.allclose(b["ftotal"], tot, rtol=0.0, atol=1e-12)
        assert a["atoms"] == b["atoms"] and np.array_equal(a["value"], b["value"])
        assert a["energy"] == pytest.approx(b["energy"], rel=1e-13)
    assert np.all(f_seq[G["b"], 0] == 0.1) and np.allclose(f_seq[G["b"], 2], (0.5 - 0.3) - 0.125, rtol=0.0, atol=1e-15)
    # what the device refuses: a slot that shares atoms with an aveforce in front of it
    bad = [slots[2], slots[0]]
    assert gforceref.shares_with_ave_in_front(bad, len(f)) == [(0, 1, int(G["b"].sum()))]
    with pytest.raises(AssertionError):
        gforceref.walk(bad, box, x, img, f.copy())


@pytest.mark.parametrize("style", STYLES)
def test_under_setforce_0_0_0_the_groups_velocities_stay_bit_for_bit(oracle, style):
    host, worst = _reference(oracle, style, "set")
    _check_reference(style, "set", host, worst)
    s, v0, by_tag, g, x_in, img = _case(style)
    l = _group(style, A_BIT)
    for step in (0,) + EVERY20:
        assert np.array_equal(host[step][2][l], v0[l]), step
        assert np.array_equal(host[step][2][~g], v0[~g]), step
    assert np.abs(host[NSTEPS][2][g & ~l] - v0[g & ~l]).max() > 0.1


_MEASURED = {}


@pytest.mark.parametrize("style", STYLES)
def test_the_order_of_the_sums_moves_the_reference_a_hundred_times_less_than_the_bounds(oracle, style, capsys):
    """The device adds a slot's atoms in its own order (per lane, per block, then the blocks); the reference with them added
    in a random order, and with math.fsum, differs from the one in the order of the cell by 100 times less than the device
    is allowed, over the four-slot case and all reads"""
    slots = _ref_slots(style, CASES["four"])
    a, worst = _reference(oracle, style, "four")
    _check_reference(style, "four", a, worst)
    assert worst["flagged"] >= 1                       # (an atom changes its image flag during the run: the energy follows it)
    s = _case(style)[0]
    wf = we = wx = wv = 0.0
    for how in ("permuted", "exact"):
        b, _ = _reference(oracle, style, "four", how=how)
        for step in (0,) + EVERY20:
            for p, q in zip(a[step][1], b[step][1]):
                assert p["atoms"] == q["atoms"]
                wf = worse(wf, float(np.abs(p["ftotal"] - q["ftotal"]).max()))
                wf = worse(wf, float(np.abs(p["value"] - q["value"]).max()))
                we = worse(we, abs(p["energy"] - q["energy"]))
            dx = b[step][0] - a[step][0]
            dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
            wx, wv = worse(wx, float(np.abs(dx).max())), worse(wv, float(np.abs(b[step][2] - a[step][2]).max()))
    with capsys.disabled():
        print(f"order of the sums, four slots ({style}): F_k {wf:.2e} eV/A, E_k {we:.2e} eV, |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps over {1 + len(EVERY20)} reads")
    assert wf > 0.0 and we > 0.0
    assert 100.0 * wf <= gforceref.F_TOL and 100.0 * we <= gforceref.E_TOL, (wf, we)
    assert 100.0 * wx < XTOL and 100.0 * wv < VTOL, (wx, wv)
