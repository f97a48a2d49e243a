"""GPU: tether springs on the device (mdp_spring_setup / _run / _state / _off; spring_sums_kernel, spring_control_kernel and
spring_apply_kernel of csrc/spring.hip in front of the kicks) against the masked host loop of tests/springref.py around the
ORACLE forces.

The two cells of tests/test_gpu_heat_mdp.py at 300 K, 200 steps of 0.001 ps with rebuild="auto" and a 0.5 A skin, the masks
of bathsref.masks (a third of the cell is held).  The image flags are handed in by tag, drawn from -2 .. 2 per dimension,
so the centre of mass of a group lies boxes away from its wrapped positions; every tether point is given relative to the
group's unwrapped centre of mass at the start.

Bounds.  Positions 1e-9 A, velocities 2e-8 A/ps, held atoms bit for bit: the project's own, from the indent and heat tests.
M and the atom counts exact.  For xcm, E and ftotal the project has no number; they come from the reference's own
sensitivity to the order of its sums (test_the_order_of_the_sums_moves_the_reference_a_hundred_times_less_than_the_bounds,
no GPU): over the two cases with the most springs (three on the alloy, four on MoS2) and all reads, the host loop with every
spring's atoms summed in a random order, and with math.fsum, moves away from the loop that sums them in the cell's order by
at most
    xcm 7.82e-14 A,   E 9.44e-12 eV,   ftotal 1.95e-12 eV/A          (measured; all three on MoS2)
and the bounds are 100 times that, rounded up in the second digit:
    xcm 7.9e-12 A,    E 9.5e-10 eV,    ftotal 2.0e-10 eV/A.
M has one value, the correctly rounded sum of the masses (math.fsum): the device forms it from two exact partial sums."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from firerig import BIG
from refloops import worse
from test_gpu_heat_mdp import _system, _oracle_engine, _context, _by_tag
from test_gpu_indent_mdp import STATIC as INDENT_STATIC, MOVING as INDENT_MOVING
import bathsref
import indentref
import langevinref
import springref

gpu = pytest.mark.gpu

GBIT = bathsref.INTEGRATE_BIT
A_BIT, B_BIT, C_BIT = bathsref.BATH_BITS
NSTEPS = 200
DT = 0.001
EVERY20 = tuple(range(20, 201, 20))
XTOL, VTOL = 1e-9, 2e-8
XCM_TOL, E_TOL, F_TOL = 7.9e-12, 9.5e-10, 2.0e-10
BIGFIRST = 2 ** 32 + 7

_CASE = {}


def _case(style):
    """(system, v0, mask by tag, integrate group, wrapped positions, image counts [n][3] in the order of s = by tag - 1)"""
    if style not in _CASE:
        s, v0 = _system(style)
        by_tag, g, groups = bathsref.masks(s)
        bathsref.check_masks(s, g, groups)
        assert np.array_equal(s.tag, np.arange(1, s.n + 1))
        # (more flags above 0 than below: the mean flag is 0.9, so a group's centre of mass lies about a box away)
        img = np.random.default_rng(77).choice(np.arange(-2, 3), size=(s.n, 3), p=(0.05, 0.1, 0.15, 0.3, 0.4))
        _CASE[style] = (s, v0, by_tag, g, S.wrap(s.box, s.x), img)
    return _CASE[style]


def _group(style, bit):
    s, v0, by_tag, g, x_in, img = _case(style)
    return None if not bit else (by_tag[s.tag] & bit) != 0


def _xcm0(style, bit):
    """the unwrapped centre of mass of the group of `bit` at the start"""
    s, v0, by_tag, g, x_in, img = _case(style)
    l = np.ones(s.n, dtype=bool) if not bit else _group(style, bit)
    m = s.mass[s.type][l]
    return (m[:, None] * springref.unwrap(s.box, x_in, img)[l]).sum(axis=0) / m.sum()


def _sp(style, bit, k, off, r0=0.0, vel=(0.0, 0.0, 0.0)):
    """a spring on the group of `bit` whose tether point starts at xcm0 + off (None: a NULL dimension)"""
    c0 = _xcm0(style, bit)
    return dict(k=k, r0=r0, c=tuple(None if o is None else float(c0[d] + o) for d, o in enumerate(off)), vel=vel, bit=bit)


def _springs(name):
    """the cases: (style, springs)"""
    if name in ("static-rebomos", "static-aeam"):
        style = name.split("-")[1]
        return style, [_sp(style, GBIT, 25.0, (5.0, -2.0, 1.5))]                       # R0 = 0 on the integrate group
    if name == "moving":                                                              # two NULL dimensions, on bath A
        return "rebomos", [_sp("rebomos", A_BIT, 40.0, (0.4, None, None), vel=(9.0, 3.0, -4.0))]
    if name == "r0big":                                                               # R0 beyond the distance: it pushes
        return "aeam", [_sp("aeam", B_BIT, 25.0, (0.6, 0.5, -0.4), r0=2.5, vel=(0.5, 0.0, 0.0))]
    if name == "shared":                                                              # two that share atoms, one on bit 0
        return "aeam", [_sp("aeam", GBIT, 12.0, (2.0, 2.0, -2.0)), _sp("aeam", A_BIT, 30.0, (None, -1.0, 0.5), vel=(0.0, -4.0, 0.0)),
                        _sp("aeam", 0, 30.0, (-2.5, 1.0, None), r0=0.5)]
    if name == "four":
        return "rebomos", [_sp("rebomos", GBIT, 25.0, (5.0, -3.0, 1.0)), _sp("rebomos", A_BIT, 40.0, (0.4, None, None), vel=(9.0, 0.0, 0.0)),
                           _sp("rebomos", B_BIT, 40.0, (-0.5, 0.8, 0.3), r0=2.0), _sp("rebomos", C_BIT, 30.0, (None, 1.2, -0.6), vel=(0.0, 2.0, 2.0))]
    raise KeyError(name)


def _ref(style, springs):
    return [dict(q, group=_group(style, q["bit"])) for q in springs]


def _ref_baths(style, cfg):
    s, v0, by_tag, g, x_in, img = _case(style)
    _, _, groups = bathsref.masks(s)
    return [(langevinref.Langevin(b["t_start"], b["t_stop"], b["damp"], b["seed"], s.mass, DT, S.FTM2V, boltz=S.BOLTZ, mvv2e=S.MVV2E,
                                  ratio=None, zero=False, tally=False), groups[k]) for k, b in enumerate(cfg)]


BATHS = (dict(t_start=300.0, t_stop=900.0, damp=0.05, seed=48271, ratio=None, zero=False, tally=False),
         dict(t_start=100.0, t_stop=100.0, damp=0.02, seed=7919, ratio=None, zero=False, tally=False))

_REF = {}


def _reference(oracle, style, name, springs, how="order", cut=None, baths=False, inds=None):
    """the host loop, once per case.  how: "order" (the cell's order), "permuted", "exact" (math.fsum)"""
    key = (style, name, how)
    if key not in _REF:
        s, v0, by_tag, g, x_in, img = _case(style)
        make, rebuild_every = _oracle_engine(oracle, style)
        orders = [np.random.default_rng(5 + k).permutation(s.n) for k in range(len(springs))] if how == "permuted" else None
        ref_inds = None if inds is None else [dict(q, group=_group(style, q.get("bit", 0))) for q in inds]
        _REF[key] = springref.host_spring(make, s, v0, img, NSTEPS, set(EVERY20), rebuild_every, g, _ref(style, springs), dt=DT,
                                          orders=orders, exact=how == "exact", cut=cut, baths=_ref_baths(style, BATHS) if baths else None,
                                          inds=ref_inds)
    return _REF[key]


def _check_reference(oracle, style, name, springs, host, worst, flags=True, **kw):
    """what the reference itself must show: every spring's force reaches 0.1 eV/A at some step, its group's centre of mass
    ends 0.01 A away from where the same loop WITHOUT the springs leaves it, and (flags) an atom of the integrate
    group changes its image flag during the run -- on both cells; the one spring on the 81 atoms of bath A of MoS2, 0.2 A
    from the nearest face, is the case that takes none across"""
    variant = "plain" + "".join(" + " + w for w in sorted(kw))
    off, _ = _reference(oracle, style, variant, [], **kw)     # (without springs every case of a cell is one and the same loop)
    s, v0, by_tag, g, x_in, img = _case(style)
    for k, q in enumerate(springs):
        assert worst["fmax"][k] >= 0.1, (name, k, worst)
        l = np.ones(s.n, dtype=bool) if not q["bit"] else _group(style, q["bit"])
        m = s.mass[s.type][l]
        xcm_off = (m[:, None] * off[NSTEPS][3][l]).sum(axis=0) / m.sum()
        moved = float(np.sqrt(((host[NSTEPS][1][k]["xcm"] - xcm_off) ** 2).sum()))
        assert moved >= 0.01, (name, k, moved)
    assert not flags or worst["flagged"] >= 1, (name, worst)


def _layout(style, tags_local, bit):
    """what the device's atom order offers the kernels: a 64-atom wave with spring, plain and held atoms; a 256-atom block
    without a spring atom; nlocal no multiple of the 1024 atoms a block of the sums kernel takes"""
    s, v0, by_tag, g, x_in, img = _case(style)
    m = by_tag[tags_local]
    sp, held = (m & bit) != 0, (m & GBIT) == 0
    plain = ~sp & ~held
    wave = any(sp[i:i + 64].any() and plain[i:i + 64].any() and held[i:i + 64].any() for i in range(0, len(m), 64))
    block = any(not sp[i:i + 256].any() for i in range(0, len(m) - 255, 256))
    return wave, block, len(m) % 1024 != 0


def _dstate(d, n):
    return [d.spring_state(k) for k in range(n)]


def _resident(style, springs, every=EVERY20, defer="mixed", first=0, cut=None, baths=False, inds=None, layout_bit=None):
    """one resident brick with the integrate group, the image flags and the springs (None: the plain run).  Reads at `every`;
    with defer="mixed" a read at a multiple of 40 finds its final half deferred (the state read completes it, pass included),
    "all" / "none": every final half deferred / none.  cut = (k, completed): mdp_spring_run behind step k and a new setup
    compute, with step k's final half pending across the call unless completed.
    {step: (x, [state of spring k], v)} by tag; step 0 holds the setup's state read TWICE"""
    s, v0, by_tag, g, x_in, img = _case(style)
    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        if baths:
            _, _, groups = bathsref.masks(s)
            d.langevin_baths([dict(b, bit=bit, natoms=int(l.sum())) for b, bit, l in zip(BATHS, (A_BIT, B_BIT), groups)], first=0, last=NSTEPS)
        d.compute(1, 0)
        out = {}
        if inds is not None:
            d.indent(inds)
        if springs is not None:
            d.spring(springs, first=first)
            out[0] = (_dstate(d, len(springs)), _dstate(d, len(springs)))
        r0 = ctx.dd_info()["reneighbors"]
        for step in range(1, NSTEPS + 1):
            ev = step in every
            df = {"mixed": (not ev) or step % 40 == 0, "all": True, "none": False}[defer]
            if cut is not None and step == cut[0]:
                df = not cut[1]
            d.step(0, 0, rebuild="auto", defer_final=df)
            if ev:
                sts = _dstate(d, len(springs)) if springs is not None else []
                d.flush()
                x, v = _by_tag(ctx, d, s)
                out[step] = (x, sts, v)
            if cut is not None and step == cut[0]:
                d.spring_run(first + step)
                d.compute(0, 0)                                 # the second run's setup
        if layout_bit is not None:
            wave, block, ragged = _layout(style, d.tags_local, layout_bit)
            assert wave, "no 64-atom wave holds spring, plain and held atoms"
            assert block, "no 256-atom block is free of spring atoms"
            assert ragged, "nlocal is a multiple of the atoms a block of the sums kernel takes"
        return out, ctx.dd_info()["reneighbors"] - r0
    finally:
        ctx.close()


def _state_errors(ref, dev):
    """(xcm, E, ftotal) errors of one spring's state, absolute; mass to rounding of the sum's order, the count exact"""
    assert dev["atoms"] == ref["atoms"], (dev["atoms"], ref["atoms"])
    return (float(np.abs(dev["xcm"] - ref["xcm"]).max()), abs(dev["energy"] - ref["energy"]),
            float(np.abs(np.asarray(dev["ftotal"]) - ref["ftotal"]).max()))


def _compare(style, host, dev, what, every=EVERY20, scale=1.0, x_in=True, first=0):
    s, v0, by_tag, g, x0, img = _case(style)
    wx = wv = wc = we = wf = 0.0
    for step in every:
        xh, sh, vh = host[step][:3]
        xd, sd, vd = dev[step]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        wx = worse(wx, float(np.abs(dx).max()))
        wv = worse(wv, float(np.abs(vd - vh).max()))
        assert len(sd) == len(sh)
        for a, b in zip(sd, sh):
            c, e, f = _state_errors(b, a)
            wc, we, wf = worse(wc, c), worse(we, e), worse(wf, f)
            if "passes" in a:                                # (a device state: mass, tether point and step are the step's)
                assert a["mass"] == b["mass"], (what, step, a["mass"], b["mass"])
                assert np.allclose(a["tether"], b["tether"], rtol=0.0, atol=1e-12), (what, step)
                assert a["step"] == first + step, (what, step, a["step"])
        assert np.array_equal(xd[~g], (x0 if x_in else xh)[~g]), (what, step, "a held atom moved")
        assert np.array_equal(vd[~g], v0[~g]), (what, step, "a held atom's velocity changed")
    print(f"{what}: worst |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps, xcm {wc:.2e} A, E {we:.2e} eV, ftotal {wf:.2e} eV/A over {len(every)} reads")
    assert wx < XTOL * scale and wv < VTOL * scale, (wx, wv)
    assert wc < XCM_TOL * scale and we < E_TOL * scale and wf < F_TOL * scale, (wc, we, wf)
    return wc, we, wf


def _same(a, b, every=EVERY20, steps=True):
    for step in every:
        assert np.array_equal(a[step][0], b[step][0]) and np.array_equal(a[step][2], b[step][2]), step
        for p, q in zip(a[step][1], b[step][1]):
            assert p["energy"] == q["energy"] and np.array_equal(p["ftotal"], q["ftotal"]) and np.array_equal(p["xcm"], q["xcm"]), step
            assert p["mass"] == q["mass"] and p["atoms"] == q["atoms"] and np.array_equal(p["tether"], q["tether"]), step
            assert not steps or (p["step"] == q["step"] and p["passes"] == q["passes"]), step


# ---- 0. the reference itself, on the CPU: where the bounds of xcm, E and ftotal come from ------------------------------------
@pytest.mark.parametrize("name", ["shared", "four"])
def test_the_order_of_the_sums_moves_the_reference_a_hundred_times_less_than_the_bounds(oracle, name, capsys):
    """no GPU.  The device adds a spring's atoms in its own order (per lane, per block, then the blocks); the reference with
    them added in a random order, and with math.fsum, differs from the one in the order of the cell by 100 times less than
    the device is allowed (the module's docstring holds the measured values)"""
    style, springs = _springs(name)
    a, wa = _reference(oracle, style, name, springs)
    _check_reference(oracle, style, name, springs, a, wa)
    for how in ("permuted", "exact"):
        b, _ = _reference(oracle, style, name, springs, how=how)
        with capsys.disabled():
            _compare(style, a, {n: (q[0], q[1], q[2]) for n, q in b.items()}, f"{how} sums, {name} ({style})", scale=0.01, x_in=False)


# ---- 1. one spring: static with R0 = 0, moving with two NULL dimensions, R0 beyond the distance ------------------------------
_DEV = {}


def _run(oracle, name, defer="mixed", **kw):
    key = (name, defer)
    if key not in _DEV:
        style, springs = _springs(name)
        _DEV[key] = _resident(style, springs, defer=defer, **kw)
    return _DEV[key]


@gpu
@pytest.mark.parametrize("name", ["static-rebomos", "static-aeam"])
def test_a_static_tether_on_the_integrate_group_follows_the_host_reference(oracle, name, capsys):
    style, springs = _springs(name)
    host, worst = _reference(oracle, style, name, springs)
    _check_reference(oracle, style, name, springs, host, worst)
    dev, renb = _run(oracle, name)
    assert renb >= 1, "the device never reneighbored: mask and image flags were not permuted"
    with capsys.disabled():
        _compare(style, host, dev, f"static tether, R0 = 0, {style} ({renb} reneighborings)")
    for step in EVERY20:
        assert dev[step][1][0]["passes"] == step + 1 and dev[step][1][0]["ftotal"][3] > 0.0
    # the state at step 0, before any kick: the reference's setup values; reading it twice changes nothing
    first, second = dev[0]
    c, e, f = _state_errors(host[0][1][0], first[0])
    assert c < XCM_TOL and e < E_TOL and f < F_TOL, (c, e, f)
    assert first[0]["step"] == 0 and first[0]["passes"] == 1 and second[0]["passes"] == 1
    _same({0: (np.zeros(1), first, np.zeros(1))}, {0: (np.zeros(1), second, np.zeros(1))}, every=(0,))
    s, v0, by_tag, g, x_in, img = _case(style)
    assert np.abs(first[0]["xcm"] - x_in[g].mean(axis=0)).max() > 0.5 * s.box.prd.min()      # a box away from the wrapped atoms


@gpu
def test_a_moving_tether_with_two_null_dimensions_follows_the_host_reference(oracle, capsys):
    style, springs = _springs("moving")
    host, worst = _reference(oracle, style, "moving", springs)
    _check_reference(oracle, style, "moving", springs, host, worst, flags=False)
    dev, renb = _run(oracle, "moving", layout_bit=A_BIT)
    with capsys.disabled():
        _compare(style, host, dev, "moving tether, y and z NULL, rebomos")
    for step in EVERY20:
        q = dev[step][1][0]
        assert not q["ftotal"][1:3].any() and not q["tether"][1:].any()
        assert q["tether"][0] == pytest.approx(springs[0]["c"][0] + 9.0 * step * DT, abs=1e-12)


@gpu
def test_a_rest_length_beyond_the_distance_pushes(oracle, capsys):
    style, springs = _springs("r0big")
    host, worst = _reference(oracle, style, "r0big", springs)
    _check_reference(oracle, style, "r0big", springs, host, worst)
    assert all(host[n][1][0]["dr"] < 0.0 for n in (0,) + EVERY20)
    dev, _ = _resident(style, springs)
    with capsys.disabled():
        _compare(style, host, dev, "R0 beyond the distance, aeam")
    assert all(dev[n][1][0]["ftotal"][3] < 0.0 for n in EVERY20) and dev[0][0][0]["ftotal"][3] < 0.0


# ---- 2. several springs -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["shared", "four"])
def test_several_springs_that_share_atoms_and_fill_the_slots(oracle, name, capsys):
    """shared: the integrate group, bath A inside it and bit 0 (every atom, the held ones included: they feel the force and
    stay).  four: the integrate group and the three baths"""
    style, springs = _springs(name)
    host, worst = _reference(oracle, style, name, springs)
    _check_reference(oracle, style, name, springs, host, worst)
    dev, _ = _resident(style, springs)
    with capsys.disabled():
        _compare(style, host, dev, f"{len(springs)} springs ({name}), {style}")
    s = _case(style)[0]
    if name == "shared":
        assert dev[NSTEPS][1][2]["atoms"] == s.n and dev[NSTEPS][1][1]["atoms"] < dev[NSTEPS][1][0]["atoms"] < s.n


# ---- 3. the step counter, deferral, two runs ----------------------------------------------------------------------------------
@gpu
def test_a_run_from_step_2_to_the_32_plus_7_is_the_run_from_0_bit_for_bit(oracle):
    style, springs = _springs("moving")
    a, _ = _run(oracle, "moving", layout_bit=A_BIT)
    b, _ = _resident(style, springs, first=BIGFIRST)
    _same(a, b, steps=False)
    for step in EVERY20:
        assert b[step][1][0]["step"] == BIGFIRST + step
    assert b[0][0][0]["step"] == BIGFIRST


@gpu
def test_deferred_and_undeferred_runs_agree_bit_for_bit_and_two_runs_are_identical(oracle):
    """REBO-MoS, whose forces are added in a fixed order.  The fused final + initial launch stays fused with the pass in
    front of it; a host that defers nothing runs the pass in front of the final half instead"""
    style, springs = _springs("moving")
    mixed, _ = _run(oracle, "moving", layout_bit=A_BIT)
    for defer in ("all", "none", "none"):
        _same(mixed, _resident(style, springs, defer=defer)[0])


@gpu
@pytest.mark.parametrize("completed", [False, True], ids=["pending", "completed"])
def test_two_runs_in_a_row_on_one_context(oracle, completed, capsys):
    """mdp_spring_run behind step 30 of 200: the tether point starts again at c.  The seam's final half is left pending
    across the call, which completes it with the pass of its step, or has run on its own: the same trajectory bit for bit"""
    k = 30
    style, springs = _springs("moving")
    host, worst = _reference(oracle, style, "two runs", springs, cut=k)
    dev, _ = _resident(style, springs, cut=(k, completed))
    with capsys.disabled():
        _compare(style, host, dev, f"two runs, seam {'completed' if completed else 'pending'}")
    q = dev[120][1][0]
    assert q["step"] == 120 and q["tether"][0] == pytest.approx(springs[0]["c"][0] + 9.0 * 90 * DT, abs=1e-12)
    key = ("two runs", not completed)
    _DEV[("two runs", completed)] = dev
    if key in _DEV:
        _same(dev, _DEV[key])


# ---- 4. next to Langevin baths, next to an indenter; off ------------------------------------------------------------------------
@gpu
def test_a_spring_next_to_two_langevin_baths(oracle, capsys):
    style, springs = _springs("static-aeam")
    host, worst = _reference(oracle, style, "baths", springs, baths=True)
    _check_reference(oracle, style, "baths", springs, host, worst, baths=True)
    dev, _ = _resident(style, springs, baths=True)
    with capsys.disabled():
        _compare(style, host, dev, "static tether next to two Langevin baths, aeam")


@gpu
def test_a_spring_next_to_an_indenter(oracle, capsys):
    """the reference adds both, the indenter first: the order of the two passes"""
    style, springs = _springs("static-aeam")
    inds = [INDENT_STATIC["aeam"]]
    host, worst = _reference(oracle, style, "indenter", springs, inds=inds)
    _check_reference(oracle, style, "indenter", springs, host, worst, inds=inds)
    assert host[0][4][0]["contacts"] == 6 and host[NSTEPS][4][0]["contacts"] >= 3        # (the indenter does push, all run long)
    dev, _ = _resident(style, springs, inds=inds)
    with capsys.disabled():
        _compare(style, host, dev, "static tether next to a spherical indenter, aeam")


def _read_both(defer, indenter_first):
    """the run of test_a_spring_next_to_an_indenter on the MoS2 cell, whose forces are added in a fixed order (the alloy's
    runs agree to rounding only), with a static and a moving sphere, and both kinds' states read at the setup and at every
    read, the indenters' before the spring's or behind it: {step: (x, v, [indenter states], [spring state])}, step 0
    without x and v"""
    style, springs = _springs("static-rebomos")
    inds = [INDENT_STATIC[style], INDENT_MOVING[style]]
    s, v0, by_tag, g, x_in, img = _case(style)
    ctx, st, cutghost, skin, map_ = _context(style)

    def states(d):
        if indenter_first:
            i = [d.indent_state(k) for k in range(len(inds))]
            return i, _dstate(d, 1)
        p = _dstate(d, 1)
        return [d.indent_state(k) for k in range(len(inds))], p

    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        d.compute(1, 0)
        d.indent(inds)
        d.spring(springs)
        out = {0: (None, None) + states(d)}
        for step in range(1, NSTEPS + 1):
            d.step(0, 0, rebuild="auto", defer_final=defer == "all")
            if step in EVERY20:
                i, p = states(d)
                d.flush()
                x, v = _by_tag(ctx, d, s)
                out[step] = (x, v, i, p)
        return out
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("defer", ["all", "none"])
def test_the_order_of_the_state_reads_of_a_spring_and_an_indenter_changes_nothing(defer):
    """a pass runs once for the forces the context holds, the indenters' first, whichever state is asked for first and
    whether the read finds the final half deferred (it completes it, passes included) or done: positions, velocities and
    every state word bit for bit, and `passes` of both kinds = the computes whose forces were consumed or read, the
    setup's and one per step"""
    a, b = _read_both(defer, True), _read_both(defer, False)
    for step in (0,) + EVERY20:
        for what, p, q in zip(("x", "v"), a[step][:2], b[step][:2]):
            assert step == 0 or np.array_equal(p, q), (defer, step, what)
        for kind, p, q in [(kind, p, q) for kind, ps, qs in zip(("indenter", "spring"), a[step][2:], b[step][2:]) for p, q in zip(ps, qs)]:
            assert p.keys() == q.keys()
            for w in p:
                assert np.array_equal(p[w], q[w]), (defer, step, kind, w, p[w], q[w])
            assert p["passes"] == step + 1 and p["step"] == step, (defer, step, kind, p["passes"], p["step"])
        assert len(a[step][2]) == len(b[step][2]) == 2 and len(a[step][3]) == len(b[step][3]) == 1
    assert sum(q["contacts"] for q in a[NSTEPS][2]) >= 1 and a[NSTEPS][3][0]["ftotal"][3] != 0.0        # (both kinds push)


_PLAIN = []


@gpu
def test_a_context_after_spring_off_is_the_plain_run_bit_for_bit():
    """off before any kick.  The state read has run the pass on the setup's forces, so the host computes them again, as the
    setup of the next run does after an unfix"""
    style, springs = _springs("moving")
    s, v0, by_tag, g, x_in, img = _case(style)
    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        d.compute(1, 0)
        d.spring(springs)
        assert d.spring_state(0)["ftotal"][3] > 0.1
        d.spring_off()
        with pytest.raises(capi.MdpError, match="mdp_spring_setup not called"):
            ctx.spring_state(0)
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
    b = _resident(style, None)[0]
    for step in EVERY20:
        assert np.array_equal(out[step][0], b[step][0]) and np.array_equal(out[step][1], b[step][2]), step


# ---- 5. a cell sheared in xz and yz: the state alone ----------------------------------------------------------------------------
@gpu
def test_the_centre_of_mass_in_a_cell_sheared_in_xz_and_yz():
    """no dynamics: the alloy cell sheared homogeneously into a box with all three tilts, read right after setup; xcm
    against springref (the image flags carry xz and yz into x and y)"""
    s0, v0 = _system("aeam")
    box = S.Box(s0.box.lo.copy(), s0.box.prd.copy(), np.array([0.35, -0.45, 0.25]))
    s = S.System(box, np.ascontiguousarray(box.lamda2x(s0.box.x2lamda(s0.x))), s0.type, s0.tag, s0.mass)
    by_tag, g, groups = bathsref.masks(s)
    img = np.random.default_rng(78).integers(-2, 3, (s.n, 3))
    assert (img[:, 2] != 0).sum() > s.n // 2
    springs = [dict(k=5.0, r0=1.0, c=(1.0, 2.0, 3.0), bit=GBIT), dict(k=5.0, r0=0.0, c=(None, 0.0, None), bit=0)]
    ctx, st, cutghost, skin, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=np.zeros((s.n, 3)))
        d.set_group(by_tag, GBIT)
        d.track_images(resident.image_pack(img))
        d.compute(0, 0)
        d.spring(springs)
        states = _dstate(d, 2)
        x = np.zeros((s.n, 3))
        x[d.tags_local - 1] = ctx.md_download(d.nlocal, want=("x",))["x"]
        imgd = np.zeros((s.n, 3), dtype=np.int64)
        imgd[d.tags_local - 1] = d.images_local()
    finally:
        ctx.close()
    ref = [dict(springs[0], group=g), dict(springs[1], group=None)]
    want = springref.post_force(ref, 0, 0, DT, s.box, x, imgd, s.mass[s.type])
    flat = springref.post_force(ref, 0, 0, DT, S.Box(box.lo, box.prd, np.array([0.35, 0.0, 0.0])), x, imgd, s.mass[s.type])
    for a, b, c in zip(states, want, flat):
        assert a["atoms"] == b["atoms"] and a["mass"] == b["mass"]
        assert np.abs(a["xcm"] - b["xcm"]).max() < XCM_TOL, (a["xcm"], b["xcm"])
        assert np.abs(b["xcm"] - c["xcm"])[:2].min() > 1e-3                 # (xz and yz do matter to it)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
@gpu
def test_library_refusals():
    style, (ok,) = _springs("moving")
    s, v0, by_tag, g, x_in, img = _case(style)
    c = capi.Context(0)
    try:
        with pytest.raises(capi.MdpError, match="0 springs; a context takes 1 to 4") as e:
            c.spring_setup([])
        assert e.value.code == -1                           # MDP_EINVAL
        with pytest.raises(capi.MdpError, match="5 springs; a context takes 1 to 4"):
            c.spring_setup([ok] * 5)
        for bad in (float("nan"), float("inf"), -1.0):
            with pytest.raises(capi.MdpError, match="spring 1: K must be finite and >= 0"):
                c.spring_setup([ok, dict(ok, k=bad)])
            with pytest.raises(capi.MdpError, match="spring 0: R0 must be finite and >= 0"):
                c.spring_setup([dict(ok, r0=bad)])
        with pytest.raises(capi.MdpError, match="spring 0: tether point and velocity must be finite"):
            c.spring_setup([dict(ok, vel=(0.0, float("nan"), 0.0))])
        with pytest.raises(capi.MdpError, match="spring 0: tether point and velocity must be finite"):
            c.spring_setup([dict(ok, c=(float("inf"), None, None))])
        with pytest.raises(capi.MdpError, match=r"spring 0: no dimension takes part \(use is all zero\)"):
            c.spring_setup([dict(ok, c=(None, None, None))])
        with pytest.raises(capi.MdpError, match="mdp_spring_setup not called") as e:
            c.spring_run(0)
        assert e.value.code == -6                           # MDP_ESTATE
        with pytest.raises(capi.MdpError, match="mdp_spring_setup not called"):
            c.spring_state(0)
        c.spring_off()                                      # (nothing is on: nothing to do)
        # a host-linked context: its host keeps the image flags
        c.rebomos_set_params(capi.read_rebomos_file(POT_REBOMOS))
        c.hnve_setup(DT, S.FTM2V, s.mass)
        with pytest.raises(capi.MdpError, match="mdp_spring_setup: springs need a resident context .* the host keeps the image flags") as e:
            c.spring_setup([ok])
        assert e.value.code == -6
    finally:
        c.close()

    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0.copy())
        d.compute(1, 0)
        with pytest.raises(capi.MdpError, match=r"mdp_spring_setup: no image set \(mdp_md_set_image\)"):
            d.spring([dict(ok, bit=0)])
        d.track_images(resident.image_pack(img))
        with pytest.raises(capi.MdpError, match="mdp_spring_setup: a spring acts on a group but no mask covers the current atoms") as e:
            d.spring([ok])
        assert e.value.code == -6
        d.spring([dict(ok, bit=0)])                         # (bit 0 needs no mask)
        d.set_group(by_tag, GBIT)
        with pytest.raises(capi.MdpError, match=r"mdp_spring_setup: spring 1 has no atoms \(group bit 64\)"):
            d.spring([ok, dict(ok, bit=64)])
        d.spring([ok, dict(ok, bit=GBIT)])
        # springs that were on stay on, as they were, after a refused setup
        before = [ctx.spring_state(k) for k in range(2)]
        for bad in ([dict(ok, k=-1.0)], [dict(ok, bit=64)], [ok] * 5):
            with pytest.raises(capi.MdpError):
                ctx.spring_setup(bad)
        after = [ctx.spring_state(k) for k in range(2)]
        for p, q in zip(before, after):
            assert p["energy"] == q["energy"] and np.array_equal(p["ftotal"], q["ftotal"]) and p["passes"] == q["passes"] == 1
        with pytest.raises(capi.MdpError, match="spring index 2 out of range"):
            ctx.spring_state(2)
        # the chain, heat sources or the minimiser, in either order
        with pytest.raises(capi.MdpError, match="mdp_nhc_setup: springs"):
            ctx.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: springs"):
            ctx.heat_setup([dict(eflux=1.0, nevery=1, bit=A_BIT)])
        with pytest.raises(capi.MdpError, match="mdp_fire_setup: springs"):
            ctx.fire_setup(0.0, 0.0, BIG, BIG)
        d.spring_off()
        ctx.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_spring_setup: the Nose-Hoover chain"):
            d.spring([ok])
        ctx.nhc_off()
        ctx.heat_setup([dict(eflux=1.0, nevery=1, bit=A_BIT)])
        with pytest.raises(capi.MdpError, match="mdp_spring_setup: heat sources"):
            d.spring([ok])
        ctx.heat_off()
        ctx.fire_setup(0.0, 0.0, BIG, BIG)
        with pytest.raises(capi.MdpError, match="mdp_spring_setup: a minimisation"):
            d.spring([ok])
        ctx.fire_off()
        d.langevin(300.0, 300.0, 0.1, 4711)                 # (a Langevin thermostat and indenters are welcome)
        d.indent([INDENT_STATIC[style]])
        d.spring([ok])
        d.spring_off()
    finally:
        ctx.close()

    # a group whose atoms have no mass: no centre of mass either
    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        s2 = S.System(s.box, s.x, s.type, s.tag, np.array([0.0, s.mass[1], 0.0]))
        d = resident.DeviceDomain(ctx, st, s2, cutghost, skin, map_, v0=np.zeros((s.n, 3)))
        mask2 = by_tag.copy()
        mask2[s.tag] |= np.where(s.type == 2, 64, 0).astype(mask2.dtype)
        d.set_group(mask2, GBIT)
        d.track_images(resident.image_pack(img))
        with pytest.raises(capi.MdpError, match=rf"mdp_spring_setup: the {int((s.type == 2).sum())} atoms of spring 1 \(group bit 64\) have no mass"):
            ctx.spring_setup([ok, dict(ok, bit=64)])
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
            d.track_images(resident.image_pack(img))
            if first:
                c.spring_setup([ok])
                with pytest.raises(capi.MdpError, match=r"mdp_dd_setup: springs \(mdp_spring_setup\) run on one rank only"):
                    c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
            else:
                c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
                with pytest.raises(capi.MdpError, match="mdp_spring_setup: springs run on one rank only"):
                    c.spring_setup([ok])
        finally:
            c.close()
