"""GPU: prescribed forces on groups on the device (mdp_gforce_setup / _run / _state / _off; gforce_sums_kernel,
gforce_control_kernel and gforce_apply_kernel of csrc/gforce.hip in front of the kicks, behind the indenters and the springs)
against the masked host loop of tests/gforceref.py around the ORACLE forces.

The two cells of tests/test_gpu_heat_mdp.py at 300 K, 200 steps of 0.001 ps with rebuild="auto" and a 0.5 A skin, the masks
of bathsref.masks (a third of the cell is held) and the image flags of tests/test_gpu_spring_mdp.py (-2 .. 2 per dimension,
so the unwrapped positions an addforce's energy is taken over lie boxes away from the wrapped ones).  The atoms of a bath
start at one velocity per bath and the integrate group without a velocity along y (_case says why).

The cases, on both pair styles: each kind alone (setforce 0 0 0 on bath A; addforce on EVERY atom, bit 0: the held atoms feel
it and stay; aveforce on bath B), setforce with one NULL, aveforce with two, four slots at once (setforce y on the integrate
group, addforce on bath A, setforce x on bath B and then aveforce y z on bath B: B's atoms are in three slots, the last of
them the aveforce), the stage behind an indenter and a spring, and next to Langevin baths on other atoms.

Bounds.  Positions 1e-9 A, velocities 2e-8 A/ps, held atoms bit for bit: the project's own, from the heat, indent and
spring tests.  Atom counts and the step word exact; what a setforce writes and an addforce adds is the number it was given.
For F_k (and the value an aveforce writes, F_k / N_k + f) and E_k the project has no number; they come from the reference's
own sensitivity to the order of its sums (tests/test_gforceref.py, no GPU): over the four-slot case of both cells and all
reads, the host loop with every slot's atoms summed in a random order, and with math.fsum, moves away from the loop that
sums them in the cell's order by at most
    F_k 1.31e-12 eV/A (MoS2; the alloy 9.24e-14),   E_k 5.68e-13 eV (MoS2; the alloy 4.55e-13)          (measured)
and the bounds are 100 times that, rounded up in the second digit (gforceref.F_TOL, gforceref.E_TOL):
    F_k 1.4e-10 eV/A,    E_k 5.7e-11 eV.
The four-slot case carries the largest energy of all cases (its addforce is the strongest), so the bound that comes from it
is not asked of a sum of larger terms."""
import math

import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from firerig import BIG
from refloops import worse
from test_gpu_heat_mdp import _oracle_engine, _context, _by_tag
from test_gpu_indent_mdp import STATIC as INDENT_STATIC
from test_gpu_spring_mdp import _case as _spring_case, _group, _sp, _ref_baths, BATHS
import bathsref
import gforceref
import oracle_bindings as ob

gpu = pytest.mark.gpu

GBIT = bathsref.INTEGRATE_BIT
A_BIT, B_BIT, C_BIT = bathsref.BATH_BITS
NSTEPS = 200
DT = 0.001
EVERY20 = tuple(range(20, 201, 20))
XTOL, VTOL = 1e-9, 2e-8
F_TOL, E_TOL = gforceref.F_TOL, gforceref.E_TOL
BIGFIRST = 2 ** 32 + 7
STYLES = ("rebomos", "aeam")
REF_SKIN = dict(rebomos=2.0, aeam=1.0)      # the skins of test_gpu_heat_mdp._oracle_engine's lists

GROUP_V = ((A_BIT, (0.5, 0.0, -0.3)), (B_BIT, (-0.3, 0.0, 0.2)), (C_BIT, (0.2, 0.0, 0.3)))
_GCASE = {}


def _case(style):
    """test_gpu_spring_mdp._case with the velocities a prescribed force goes with.  An atom whose force a setforce or an
    aveforce replaces moves on at its own velocity, and a thermal one would stream through the lattice, faster than the
    reference's list, built every 25 or 50 steps, allows for (gforceref.host_gforce asserts that it holds).  So every atom of
    bath A, B and C starts at its bath's velocity -- a grip or a slab moves as one piece -- and no atom of the integrate
    group has a velocity along y, the dimension the four-slot case takes the forces off for all of them"""
    if style not in _GCASE:
        s, v0, by_tag, g, x_in, img = _spring_case(style)
        v0 = v0.copy()
        v0[g, 1] = 0.0
        for bit, vel in GROUP_V:
            v0[_group(style, bit)] = vel
        _GCASE[style] = (s, v0, by_tag, g, x_in, img)
    return _GCASE[style]


CASES = {
    "set": [dict(kind="set", f=(0.0, 0.0, 0.0), bit=A_BIT)],
    "add": [dict(kind="add", f=(0.005, -0.003, 0.002), bit=0)],
    "ave": [dict(kind="ave", f=(0.05, -0.02, 0.04), bit=B_BIT)],
    "set-null": [dict(kind="set", f=(0.02, None, -0.02), bit=A_BIT)],
    "ave-null": [dict(kind="ave", f=(None, None, -0.05), bit=C_BIT)],
    "four": [dict(kind="set", f=(None, 0.0, None), bit=GBIT), dict(kind="add", f=(0.3, -0.02, 0.1), bit=A_BIT),
             dict(kind="set", f=(0.05, None, None), bit=B_BIT), dict(kind="ave", f=(None, 0.03, -0.04), bit=B_BIT)],
    "setave": [dict(kind="set", f=(0.0, 0.0, 0.0), bit=A_BIT), dict(kind="set", f=(0.05, None, None), bit=B_BIT),
               dict(kind="ave", f=(None, 0.03, -0.04), bit=B_BIT)],
    "measure": [dict(kind="set", f=(None, None, None), bit=GBIT)],
    "outside": [dict(kind="set", f=(0.0, None, None), bit=C_BIT), dict(kind="ave", f=(None, 0.02, None), bit=C_BIT)],
}


def _ref_slots(style, slots):
    return [dict(q, group=_group(style, q["bit"])) for q in slots]


def _extras(style, loaded):
    """the indenter and the spring of the `loaded` runs: (device lists, reference lists)"""
    if not loaded:
        return None, None, None, None
    inds = [INDENT_STATIC[style]]
    springs = [_sp(style, GBIT, 25.0, (5.0, -2.0, 1.5))]
    return (inds, springs, [dict(q, group=_group(style, q.get("bit", 0))) for q in inds],
            [dict(q, group=_group(style, q["bit"])) for q in springs])


_REF = {}


def _reference(oracle, style, name, how="order", cut=None, baths=False, loaded=False):
    """the host loop, once per case.  how: "order" (the cell's order), "permuted", "exact" (math.fsum)"""
    key = (style, name, how, cut, baths, loaded)
    if key not in _REF:
        s, v0, by_tag, g, x_in, img = _case(style)
        slots = CASES[name]
        make, rebuild_every = _oracle_engine(oracle, style)
        orders = [np.random.default_rng(5 + k).permutation(s.n) for k in range(len(slots))] if how == "permuted" else None
        _, _, rinds, rsprings = _extras(style, loaded)
        _REF[key] = gforceref.host_gforce(make, s, v0, img, NSTEPS, set(EVERY20), rebuild_every, g, _ref_slots(style, slots), dt=DT,
                                          orders=orders, exact=how == "exact", cut=cut, baths=_ref_baths(style, BATHS) if baths else None,
                                          inds=rinds, springs=rsprings, skin=REF_SKIN[style])
    return _REF[key]


def _layout(style, tags_local, two, one):
    """what the device's atom order offers the kernels: a 64-atom wave with atoms of two slots, of one slot and of none; a
    256-atom block without a slot atom; nlocal no multiple of the 1024 atoms a block of the sums kernel takes"""
    s, v0, by_tag, g, x_in, img = _case(style)
    m = by_tag[tags_local]
    a, b = (m & two) != 0, (m & one) != 0
    none = ~a & ~b
    wave = any(a[i:i + 64].any() and b[i:i + 64].any() and none[i:i + 64].any() for i in range(0, len(m), 64))
    block = any(none[i:i + 256].all() for i in range(0, len(m) - 255, 256))
    return wave, block, len(m) % 1024 != 0


def _dstate(d, n):
    return [d.gforce_state(k) for k in range(n)]


def _resident(style, slots, every=EVERY20, defer="mixed", first=0, cut=None, baths=False, loaded=False, layout=None):
    """one resident brick with the integrate group, the image flags and the slots (None: the plain run).  Reads at `every`;
    with defer="mixed" a read at a multiple of 40 finds its final half deferred (the state read completes it, pass included),
    "all" / "none": every final half deferred / none.  cut = (k, completed): mdp_gforce_run behind step k and a new setup
    compute, with step k's final half pending across the call unless completed.
    {step: (x, [state of slot k], v)} by tag; step 0 holds the setup's state read TWICE"""
    s, v0, by_tag, g, x_in, img = _case(style)
    ctx, st, cutghost, skin, map_ = _context(style)
    inds, springs, _, _ = _extras(style, loaded)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        if baths:
            _, _, groups = bathsref.masks(s)
            d.langevin_baths([dict(b, bit=bit, natoms=int(l.sum())) for b, bit, l in zip(BATHS, (A_BIT, B_BIT), groups)], first=0, last=NSTEPS)
        d.compute(1, 0)
        out = {}
        if loaded:
            d.indent(inds)
            d.spring(springs)
        if slots is not None:
            d.gforce(slots, first=first)
            out[0] = (_dstate(d, len(slots)), _dstate(d, len(slots)))
        if layout is not None:
            wave, block, ragged = _layout(style, d.tags_local, *layout)
            assert wave, "no 64-atom wave holds atoms of two slots, of one slot and of none"
            assert block, "no 256-atom block is free of slot atoms"
            assert ragged, "nlocal is a multiple of the atoms a block of the sums kernel takes"
        r0 = ctx.dd_info()["reneighbors"]
        for step in range(1, NSTEPS + 1):
            ev = step in every
            df = {"mixed": (not ev) or step % 40 == 0, "all": True, "none": False}[defer]
            if cut is not None and step == cut[0]:
                df = not cut[1]
            d.step(0, 0, rebuild="auto", defer_final=df)
            if ev:
                sts = _dstate(d, len(slots)) if slots is not None else []
                d.flush()
                x, v = _by_tag(ctx, d, s)
                out[step] = (x, sts, v)
            if cut is not None and step == cut[0]:
                d.gforce_run(first + step)
                if loaded:
                    d.indent_run(first + step)
                    d.spring_run(first + step)
                d.compute(0, 0)                                 # the second run's setup
        return out, ctx.dd_info()["reneighbors"] - r0
    finally:
        ctx.close()


def _state_errors(slot, ref, dev):
    """(F_k, E_k) errors of one slot's state, absolute; the count exact; the value word: the number given (set, add) or the
    reference's average to the bound of F_k"""
    assert dev["atoms"] == ref["atoms"], (dev["atoms"], ref["atoms"])
    value = np.asarray(dev["value"])
    if slot["kind"] == "ave":
        assert np.abs(value - ref["value"]).max() < F_TOL, (value, ref["value"])
    else:
        assert np.array_equal(value, gforceref.values(slot)), (value, slot)
    if slot["kind"] != "add":
        assert dev["energy"] == 0.0
    return float(np.abs(np.asarray(dev["ftotal"]) - ref["ftotal"]).max()), abs(dev["energy"] - ref["energy"])


def _compare(style, slots, host, dev, what, every=EVERY20, scale=1.0, x_in=True, first=0):
    s, v0, by_tag, g, x0, img = _case(style)
    wx = wv = wf = we = 0.0
    for step in every:
        xh, sh, vh = host[step][:3]
        xd, sd, vd = dev[step]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        wx = worse(wx, float(np.abs(dx).max()))
        wv = worse(wv, float(np.abs(vd - vh).max()))
        assert len(sd) == len(sh) == len(slots)
        for q, a, b in zip(slots, sd, sh):
            f, e = _state_errors(q, b, a)
            wf, we = worse(wf, f), worse(we, e)
            if "passes" in a:                                # (a device state)
                assert a["step"] == first + step, (what, step, a["step"])
        assert np.array_equal(xd[~g], (x0 if x_in else xh)[~g]), (what, step, "a held atom moved")
        assert np.array_equal(vd[~g], v0[~g]), (what, step, "a held atom's velocity changed")
    print(f"{what}: worst |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps, F_k {wf:.2e} eV/A, E_k {we:.2e} eV over {len(every)} reads")
    assert wx < XTOL * scale and wv < VTOL * scale, (wx, wv)
    assert wf < F_TOL * scale and we < E_TOL * scale, (wf, we)
    return wf, we


def _same(a, b, every=EVERY20, steps=True):
    for step in every:
        assert np.array_equal(a[step][0], b[step][0]) and np.array_equal(a[step][2], b[step][2]), step
        for p, q in zip(a[step][1], b[step][1]):
            assert p["energy"] == q["energy"] and np.array_equal(p["ftotal"], q["ftotal"]) and np.array_equal(p["value"], q["value"]), step
            assert p["atoms"] == q["atoms"], step
            assert not steps or (p["step"] == q["step"] and p["passes"] == q["passes"]), step


_DEV = {}


def _run(style, name, defer="mixed", **kw):
    key = (style, name, defer)
    if key not in _DEV:
        _DEV[key] = _resident(style, CASES[name], defer=defer, **kw)
    return _DEV[key]


def _check_reference(style, name, host, worst):
    """what the reference itself must show: every slot's group force reaches 0.01 eV/A at some step -- but for a slot on
    every atom: the pair forces add up to nothing there, to rounding"""
    for k, q in enumerate(CASES[name]):
        assert (worst["fmax"][k] >= 0.01) == (q["bit"] != 0) and (q["bit"] != 0 or worst["fmax"][k] < 1e-10), (style, name, k, worst)


# ---- 1. each kind alone, NULL dimensions ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", ["set", "add", "ave", "set-null", "ave-null"])
def test_one_slot_follows_the_host_reference(oracle, style, name, capsys):
    slots = CASES[name]
    host, worst = _reference(oracle, style, name)
    _check_reference(style, name, host, worst)
    dev, renb = _run(style, name)
    assert renb >= 1, "the device never reneighbored: mask and image flags were not permuted"
    with capsys.disabled():
        _compare(style, slots, host, dev, f"{name}, {style} ({renb} reneighborings)")
    for step in EVERY20:
        assert dev[step][1][0]["passes"] == step + 1
    # the state at step 0, before any kick: the reference's setup values; reading it twice changes nothing
    first, second = dev[0]
    f, e = _state_errors(slots[0], host[0][1][0], first[0])
    assert f < F_TOL and e < E_TOL, (f, e)
    assert first[0]["step"] == 0 and first[0]["passes"] == 1 and second[0]["passes"] == 1
    _same({0: (np.zeros(1), first, np.zeros(1))}, {0: (np.zeros(1), second, np.zeros(1))}, every=(0,))
    s, v0, by_tag, g, x_in, img = _case(style)
    if name == "set":               # setforce 0 0 0: the group's velocities never change, and it moves
        l = _group(style, A_BIT)
        for step in EVERY20:
            assert np.array_equal(dev[step][2][l], v0[l]), step
        assert np.abs(dev[NSTEPS][0][l] - x_in[l]).max() > 0.05
    if name == "add":               # bit 0: every atom is in the group, the held ones included; the energy is of the unwrapped positions
        assert first[0]["atoms"] == s.n
        wrapped = -float((x_in @ np.array(slots[0]["f"])).sum())
        assert abs(first[0]["energy"] - wrapped) > 1.0
    if name == "ave-null":
        assert not np.asarray(dev[NSTEPS][1][0]["value"])[:2].any() and dev[NSTEPS][1][0]["value"][2] != 0.0


# ---- 2. several slots ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("style", STYLES)
def test_four_slots_that_share_atoms(oracle, style, capsys):
    """setforce y on the integrate group, addforce on bath A, setforce x on bath B and then aveforce y z on bath B: an atom
    of B walks three slots, the aveforce last; its y average is taken over what the first setforce wrote"""
    slots = CASES["four"]
    host, worst = _reference(oracle, style, "four")
    _check_reference(style, "four", host, worst)
    dev, _ = _run(style, "four")
    with capsys.disabled():
        _compare(style, slots, host, dev, f"four slots, {style}")
    for step in EVERY20:
        ave = dev[step][1][3]
        assert ave["value"][0] == 0.0 and ave["value"][1] == 0.03          # (the average of zeros, plus f)
        assert ave["ftotal"][1] == 0.0 and ave["ftotal"][0] != 0.0


@gpu
@pytest.mark.parametrize("style", STYLES)
def test_the_stage_behind_an_indenter_and_a_spring(oracle, style, capsys):
    """the reference applies the indenter, then the spring, then the slots: a setforce overwrites what the two added.  The
    device's atom order offers a wave with atoms of two slots (bath B), of one (bath A) and of none, and a block of none"""
    slots = CASES["setave"]
    host, worst = _reference(oracle, style, "setave", loaded=True)
    _check_reference(style, "setave", host, worst)
    bare, _ = _reference(oracle, style, "setave")
    assert np.abs(bare[NSTEPS][1][0]["ftotal"] - host[NSTEPS][1][0]["ftotal"]).max() > 10 * F_TOL     # (the two do push on the slots' atoms)
    dev, _ = _resident(style, slots, loaded=True, layout=(B_BIT, A_BIT))
    with capsys.disabled():
        _compare(style, slots, host, dev, f"set, set and ave behind an indenter and a spring, {style}")


@gpu
@pytest.mark.parametrize("style", STYLES)
def test_next_to_langevin_baths_on_other_atoms(oracle, style, capsys):
    """baths on A and B, setforce x and aveforce y on C"""
    slots = CASES["outside"]
    host, worst = _reference(oracle, style, "outside", baths=True)
    _check_reference(style, "outside", host, worst)
    dev, _ = _resident(style, slots, baths=True)
    with capsys.disabled():
        _compare(style, slots, host, dev, f"set and ave next to two Langevin baths, {style}")


# ---- 3. the step counter, deferral, two runs, the plain run ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("style", STYLES)
def test_a_run_from_step_2_to_the_32_plus_7_is_the_run_from_0(oracle, style):
    a, _ = _run(style, "ave")
    b, _ = _resident(style, CASES["ave"], first=BIGFIRST)
    if style == "rebomos":      # (its forces are added in a fixed order; the alloy's runs agree to rounding only)
        _same(a, b, steps=False)
    for step in EVERY20:
        assert b[step][1][0]["step"] == BIGFIRST + step and b[step][1][0]["passes"] == step + 1
    assert b[0][0][0]["step"] == BIGFIRST


@gpu
def test_deferred_and_undeferred_runs_agree_bit_for_bit_and_two_runs_are_identical(oracle):
    """REBO-MoS, whose forces are added in a fixed order; the four slots.  The fused final + initial launch stays fused with
    the pass in front of it; a host that defers nothing runs the pass in front of the final half instead"""
    mixed, _ = _run("rebomos", "four")
    for defer in ("all", "none", "none"):
        _same(mixed, _resident("rebomos", CASES["four"], defer=defer)[0])


@gpu
@pytest.mark.parametrize("completed", [False, True], ids=["pending", "completed"])
def test_two_runs_in_a_row_on_one_context(oracle, completed, capsys):
    """mdp_gforce_run behind step 30 of 200, the seam's final half pending across the call or completed"""
    k = 30
    host, worst = _reference(oracle, "rebomos", "setave", cut=k)
    dev, _ = _resident("rebomos", CASES["setave"], cut=(k, completed))
    with capsys.disabled():
        _compare("rebomos", CASES["setave"], host, dev, f"two runs, seam {'completed' if completed else 'pending'}")
    key = ("two runs", not completed)
    _DEV[("two runs", completed)] = dev
    if key in _DEV:
        _same(dev, _DEV[key])


_PLAIN = {}


@gpu
def test_an_all_null_setforce_is_the_plain_run_bit_for_bit_while_its_sums_are_read(oracle):
    if "rebomos" not in _PLAIN:
        _PLAIN["rebomos"] = _resident("rebomos", None)[0]
    plain = _PLAIN["rebomos"]
    dev, _ = _run("rebomos", "measure")
    s, v0, by_tag, g, x_in, img = _case("rebomos")
    for step in EVERY20:
        assert np.array_equal(dev[step][0], plain[step][0]) and np.array_equal(dev[step][2], plain[step][2]), step
        q = dev[step][1][0]
        assert q["atoms"] == int(g.sum()) and np.abs(q["ftotal"]).max() > 0.0 and not np.asarray(q["value"]).any()
    host, _ = _reference(oracle, "rebomos", "measure")
    _compare("rebomos", CASES["measure"], host, dev, "all-NULL setforce")


@gpu
def test_a_context_after_gforce_off_is_the_plain_run_bit_for_bit():
    style = "rebomos"
    s, v0, by_tag, g, x_in, img = _case(style)
    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        d.compute(1, 0)
        d.gforce(CASES["four"])
        assert d.gforce_state(3)["atoms"] > 0
        d.gforce_off()
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup not called"):
            ctx.gforce_state(0)
        d.compute(1, 0)
        out = {}
        for step in range(1, NSTEPS + 1):
            ev = step in EVERY20
            d.step(0, 0, rebuild="auto", defer_final=(not ev) or step % 40 == 0)
            if ev:
                d.flush()
                out[step] = _by_tag(ctx, d, s)
    finally:
        ctx.close()
    if style not in _PLAIN:
        _PLAIN[style] = _resident(style, None)[0]
    for step in EVERY20:
        assert np.array_equal(out[step][0], _PLAIN[style][step][0]) and np.array_equal(out[step][1], _PLAIN[style][step][2]), step


# ---- 4. host-linked mode: setforce and aveforce -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("style", STYLES)
def test_hostlinked_set_and_ave_from_shuffled_atoms(oracle, style, capsys):
    """mdp_hnve_* with mdp_hnve_set_mask: the host's atom order is a shuffle of the tags, host reneighborings every 50 steps
    re-upload atoms, velocities and mask (each upload counts the sharing rule again).  Same reference, same bounds"""
    import ctypes as C
    s, v0, by_tag, g, x_in, img = _case(style)
    slots = CASES["setave"]
    host, _ = _reference(oracle, style, "setave")
    perm = np.random.default_rng(17).permutation(s.n)
    type_p, tag_p = s.type[perm].copy(), s.tag[perm].copy()
    mask_p = by_tag[tag_p]
    gp = g[perm]
    skin = 2.0 if style == "rebomos" else 1.0
    c = capi.Context(0)
    try:
        if style == "rebomos":
            P = oracle.rebomos_params(POT_REBOMOS)
            c.rebomos_set_params(ob.product_rebomos_params(P))
            cut = P.cut3rebo + skin
        else:
            af = capi.AeamFile(POT_AEAM)
            tabs = af.build()
            c.aeam_set_tables(tabs)
            c.aeam_device_lists(True)
            cut = float(af.cut_table(tabs).max()) + skin

        def upload(x, v):
            xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), type_p, tag_p, s.mass), cut)
            c.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=[0, 0, 1] if style == "rebomos" else None)
            c.set_skin(skin)
            c.hnve_upload_v(v)

        def compute():
            if style == "rebomos":
                c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
            else:
                eng, vir = C.c_double(0.0), np.zeros(6)
                c._ck(c.L.mdp_aeam_density_host(c.h, C.c_int(0), None, None, C.byref(eng), None))
                c._ck(c.L.mdp_aeam_force_host(c.h, C.c_int(0), C.c_int(0), None, None, C.byref(eng), capi._dp(vir), None, None))
        c.set_box_host(s.box)
        c.hnve_setup(DT, S.FTM2V, s.mass)
        c.integrate_group(GBIT)
        upload(x_in[perm].copy(), v0[perm])
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: a group force acts on a group but no mask covers the current atoms"):
            c.gforce_setup(slots)
        c.hnve_set_mask(mask_p)
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: an addforce needs a resident context .* the host keeps the image flags"):
            c.gforce_setup(CASES["add"])
        compute()
        c.gforce_setup(slots)
        c.gforce_run(0)
        dev, uploads = {}, 0
        for step in range(1, NSTEPS + 1):
            moved, late = c.hnve_initial()
            if moved or step % 50 == 0:     # the host's reneighboring: atoms come up, are wrapped and go down again, mask included
                got = c.hnve_download(s.n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]
                upload(xw, got["v"])
                c.hnve_set_mask(mask_p)
                uploads += 1
            compute()
            c.hnve_final()
            if step in EVERY20:
                sts = [c.gforce_state(k) for k in range(len(slots))]
                got = c.hnve_download(s.n, want=("x", "v"))
                xd, vd = np.zeros((s.n, 3)), np.zeros((s.n, 3))
                xd[tag_p - 1], vd[tag_p - 1] = got["x"], got["v"]
                dev[step] = (xd, sts, vd)
    finally:
        c.close()
    assert uploads >= 3
    with capsys.disabled():
        _compare(style, slots, host, dev, f"set, set and ave, host-linked {style}, shuffled host order ({uploads} uploads)")


# ---- 5. 275 684 atoms: the control workgroup's second trip ----------------------------------------------------------------------------
@gpu
def test_the_control_workgroups_second_trip_against_fsum(capsys):
    """275 684 aluminium atoms (fcc 41^3), each moved by up to 0.05 A so that it feels a force: gforce_sums_kernel leaves 270
    partial slots, so mdp_slot_sum_256<kGfW> of the control workgroup takes a second trip, and the last block holds 228
    atoms: its first j only.  One pass, on the forces of the setup: setforce x on tag % 8 == 1, addforce on tag % 8 == 2,
    setforce y and then aveforce x z on tag % 8 == 5, inside an integrate group that leaves tag % 7 == 0 held.
    F_k and E_k against math.fsum over the forces downloaded before the pass.  A term goes through at most 22 additions on
    the device (4 in its lane, 6 across the wave, 2 across the block, up to 2 over the partial slots and 8 down the tree),
    each with a relative error of 2^-53, so the sum differs from the exact one by no more than 22 x 2^-53 times the sum of
    the terms' magnitudes; E_k's terms f . xu carry three roundings of their own on the device and three in this test on top.  The forces behind the pass: what a
    setforce writes and an addforce adds bit for bit, the aveforce's value word on every atom of its group, every other
    word the one downloaded before."""
    af = capi.AeamFile(POT_AEAM)
    s = S.fcc_cell(4.045, 41)
    s.mass[1:3] = af.mass[:2]
    assert s.n == 275684 and -(-s.n // 1024) == 270 and s.n % 1024 == 228
    rng = np.random.default_rng(96)
    s = S.System(s.box, s.x + rng.uniform(-0.05, 0.05, s.x.shape), s.type, s.tag, s.mass)
    g = s.tag % 7 != 0
    groups = [g & (s.tag % 8 == r) for r in (1, 2, 5)]
    bits = (4, 8, 16)
    by_tag = np.zeros(s.n + 1, dtype=np.int32)
    m = bathsref.ALL_BIT | np.where(g, GBIT, 0)
    for bit, l in zip(bits, groups):
        m = m | np.where(l, bit, 0)
    by_tag[s.tag] = m
    img = rng.integers(-2, 3, (s.n, 3))
    slots = [dict(kind="set", f=(0.01, None, None), bit=bits[0]), dict(kind="add", f=(0.02, -0.01, 0.03), bit=bits[1]),
             dict(kind="set", f=(None, 0.0, None), bit=bits[2]), dict(kind="ave", f=(0.01, None, -0.02), bit=bits[2])]
    ctx, st, cutghost, skin, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=np.zeros((s.n, 3)))
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        d.compute(0, 0)
        tags = d.tags_local
        before = ctx.md_download(d.nlocal, want=("f",))["f"]
        xu = d.unwrapped_local()
        d.gforce(slots)
        states = _dstate(d, 4)
        after = ctx.md_download(d.nlocal, want=("f",))["f"]
    finally:
        ctx.close()
    u = 2.0 ** -53
    member = [groups[k][tags - 1] for k in (0, 1, 2, 2)]
    want = before.copy()
    worst = dict(F=0.0, E=0.0)
    for k, (q, l) in enumerate(zip(slots, member)):
        stt = states[k]
        assert stt["atoms"] == int(l.sum()) and stt["passes"] == 1 and stt["step"] == 0
        F = np.array([math.fsum(want[l, c]) for c in range(3)])
        bound = 22 * u * np.abs(want[l]).sum(axis=0)
        assert np.all(np.abs(stt["ftotal"] - F) <= bound), (k, stt["ftotal"], F, bound)
        worst["F"] = max(worst["F"], float((np.abs(stt["ftotal"] - F)[bound > 0.0] / bound[bound > 0.0]).max()))
        val, use = gforceref.values(q), gforceref.used(q)
        if q["kind"] == "set":
            want[np.ix_(np.flatnonzero(l), np.flatnonzero(use))] = val[use]
            assert np.array_equal(stt["value"], val)
        elif q["kind"] == "add":
            terms = xu[l] @ val
            E = -math.fsum(terms)
            ebound = (22 + 6) * u * float(np.abs(xu[l] * val).sum())
            assert abs(stt["energy"] - E) <= ebound, (stt["energy"], E, ebound)
            worst["E"] = abs(stt["energy"] - E) / ebound
            want[l] += val
            assert np.array_equal(stt["value"], val)
        else:
            ave = F / stt["atoms"] + val
            slack = bound / stt["atoms"] + 4 * u * (np.abs(F / stt["atoms"]) + np.abs(val))    # (the division and the addition, here and there)
            assert np.all(np.abs(stt["value"] - ave)[use] <= slack[use]), (stt["value"], ave)
            assert stt["value"][1] == 0.0
            want[np.ix_(np.flatnonzero(l), np.flatnonzero(use))] = np.asarray(stt["value"])[use]
    assert np.array_equal(after, want), int((after != want).any(axis=1).sum())
    other = ~np.logical_or.reduce(member)
    assert np.array_equal(after[other], before[other])
    with capsys.disabled():
        print(f"275 684 atoms, four slots against fsum: F_k at {worst['F']:.2f} of its bound, E_k at {worst['E']:.2f}")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
@gpu
def test_library_refusals():
    style = "rebomos"
    ok = CASES["ave"][0]
    s, v0, by_tag, g, x_in, img = _case(style)
    c = capi.Context(0)
    try:
        with pytest.raises(capi.MdpError, match="0 group forces; a context takes 1 to 4") as e:
            c.gforce_setup([])
        assert e.value.code == -1                           # MDP_EINVAL
        with pytest.raises(capi.MdpError, match="5 group forces; a context takes 1 to 4"):
            c.gforce_setup([ok] * 5)
        with pytest.raises(capi.MdpError, match=r"group force 1: kind 3 is none of set \(0\), add \(1\), ave \(2\)"):
            c.gforce_setup([ok, dict(ok, kind=3)])
        for bad in (float("nan"), float("inf")):
            with pytest.raises(capi.MdpError, match=r"group force 0: f\[1\] must be finite"):
                c.gforce_setup([dict(ok, f=(0.0, bad, None))])
        with pytest.raises(capi.MdpError, match=r"group force 0: an addforce takes all three dimensions \(use\[2\] is 0\)") as e:
            c.gforce_setup([dict(kind="add", f=(0.0, 0.0, None), bit=0)])
        assert e.value.code == -1
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup not called") as e:
            c.gforce_run(0)
        assert e.value.code == -6                           # MDP_ESTATE
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup not called"):
            c.gforce_state(0)
        c.gforce_off()                                      # (nothing is on: nothing to do)
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: no integrator on the context"):
            c.gforce_setup([ok])
    finally:
        c.close()

    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0.copy())
        d.compute(1, 0)
        with pytest.raises(capi.MdpError, match=r"mdp_gforce_setup: an addforce is among the group forces and no image is set \(mdp_md_set_image\)"):
            d.gforce(CASES["add"])
        d.gforce([dict(ok, bit=0)])                         # (set and ave need no image flags, and bit 0 no mask)
        d.gforce_off()
        d.track_images(resident.image_pack(img))
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: a group force acts on a group but no mask covers the current atoms") as e:
            d.gforce([ok])
        assert e.value.code == -6
        d.gforce(CASES["add"])
        d.set_group(by_tag, GBIT)
        with pytest.raises(capi.MdpError, match=r"mdp_gforce_setup: group force 1 has no atoms \(group bit 64\)"):
            d.gforce([ok, dict(ok, bit=64)])
        # what follows an aveforce must not share atoms with it: the count and both slots
        nb = int(_group(style, B_BIT).sum())
        with pytest.raises(capi.MdpError, match=rf"mdp_gforce_setup: {nb} atoms of group force 2 are also in group force 0, an aveforce in front of it") as e:
            d.gforce([ok, CASES["set"][0], dict(kind="set", f=(0.0, None, None), bit=GBIT)])
        assert e.value.code == -6
        with pytest.raises(capi.MdpError, match=rf"{nb} atoms of group force 1 are also in group force 0, an aveforce"):
            d.gforce([ok, dict(ok, f=(None, 0.0, None))])
        d.gforce(CASES["four"])
        # slots that were on stay on, as they were, after a refused setup
        before = [ctx.gforce_state(k) for k in range(4)]
        for bad in ([dict(ok, f=(float("nan"), 0.0, 0.0))], [dict(ok, bit=64)], [ok] * 5, [ok, dict(ok, bit=GBIT)]):
            with pytest.raises(capi.MdpError):
                ctx.gforce_setup(bad)
        after = [ctx.gforce_state(k) for k in range(4)]
        for p, q in zip(before, after):
            assert p["energy"] == q["energy"] and np.array_equal(p["ftotal"], q["ftotal"]) and p["passes"] == q["passes"] == 1
            assert p["atoms"] == q["atoms"] and np.array_equal(p["value"], q["value"])
        with pytest.raises(capi.MdpError, match="group force index 4 out of range"):
            ctx.gforce_state(4)
        # a mask upload while the stage is on counts the sharing again, as one does under heat sources: the call fails
        d.gforce([ok, CASES["set"][0]])
        clash = by_tag.copy()
        clash[s.tag] |= np.where(_group(style, B_BIT), A_BIT, 0).astype(clash.dtype)
        with pytest.raises(capi.MdpError, match=rf"mdp_md_set_mask: {nb} atoms of group force 1 are also in group force 0, an aveforce"):
            ctx.md_set_mask(clash[d.tags_local])
        with pytest.raises(capi.MdpError, match=rf"integrate: {nb} atoms of group force 1 are also in group force 0"):
            ctx.gforce_state(0)
        ctx.md_set_mask(by_tag[d.tags_local])
        assert ctx.gforce_state(0)["atoms"] == nb
        # the chain, heat sources or the minimiser, in either order
        with pytest.raises(capi.MdpError, match="mdp_nhc_setup: group forces"):
            ctx.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: group forces"):
            ctx.heat_setup([dict(eflux=1.0, nevery=1, bit=A_BIT)])
        with pytest.raises(capi.MdpError, match="mdp_fire_setup: group forces"):
            ctx.fire_setup(0.0, 0.0, BIG, BIG)
        d.gforce_off()
        ctx.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: the Nose-Hoover chain"):
            d.gforce([ok])
        ctx.nhc_off()
        ctx.heat_setup([dict(eflux=1.0, nevery=1, bit=A_BIT)])
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: heat sources"):
            d.gforce([ok])
        ctx.heat_off()
        ctx.fire_setup(0.0, 0.0, BIG, BIG)
        with pytest.raises(capi.MdpError, match="mdp_gforce_setup: a minimisation"):
            d.gforce([ok])
        ctx.fire_off()
        d.langevin(300.0, 300.0, 0.1, 4711)                 # (a Langevin thermostat, indenters and springs are welcome)
        d.indent([INDENT_STATIC[style]])
        d.spring([_sp(style, GBIT, 25.0, (5.0, -2.0, 1.5))])
        d.gforce([ok])
        # a refusal leaves the stages that were on as they were
        with pytest.raises(capi.MdpError):
            ctx.gforce_setup([dict(ok, bit=64)])
        assert ctx.gforce_state(0)["atoms"] == nb and ctx.spring_state(0)["atoms"] == int(g.sum()) and ctx.indent_state(0)["passes"] == 1
        d.gforce_off()
    finally:
        ctx.close()

    # a brick of several ranks, in either call order
    p = capi.read_rebomos_file(POT_REBOMOS)
    cutghost = 3.0 * p.rcmax[0][0] + 2.0
    for first in (True, False):
        c = capi.Context(0)
        try:
            c.rebomos_set_params(p)
            d = resident.DeviceDomain(c, capi.STYLE_REBOMOS, s, cutghost, 2.0, [0, 0, 1], v0=v0.copy())
            d.set_group(by_tag, GBIT)
            if first:
                c.gforce_setup([ok])
                with pytest.raises(capi.MdpError, match=r"mdp_dd_setup: group forces \(mdp_gforce_setup\) run on one rank only"):
                    c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
            else:
                c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
                with pytest.raises(capi.MdpError, match="mdp_gforce_setup: group forces run on one rank only"):
                    c.gforce_setup([ok])
        finally:
            c.close()

