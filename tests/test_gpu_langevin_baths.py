"""GPU: several Langevin baths on disjoint groups in one run (mdp_langevin_baths, mdp_langevin_tally_bath; the
LANGEVIN = MDP_LANGEVIN_MAXBATH instantiations of nve_advance_kernel, lgv_final_kernel<4, true> and the four-slot
instantiations of the zero / mean / tally kernels) against the masked host loop of tests/bathsref.py around the ORACLE forces.

The two cells of the thermostat tests at 300 K, 200 steps of 0.001 ps with rebuild="auto" and the 0.5 A skin of the group
tests.  The masks (bathsref.masks): bit 1 everywhere, integrate bit 2 as in the group tests, the baths on bits 4 / 8 / 16
inside it, integrated atoms in no bath, held atoms.  The three baths:
    A  300 -> 900 K, damp 0.05, seed 48271, scale {1: 2.0, 2: 0.5}, zero yes, tally yes
    B  100 -> 100 K, damp 0.02, seed 7919,                          zero no,  tally yes
    C  600 -> 200 K, damp 0.1,  seed 48271 (A's: the tags differ),  zero yes, tally no
The fourth slot (bathsref.masks4: bath D on bit 32, cut out of what the three leave unthermostatted):
    D  200 -> 500 K, damp 0.03, seed 104729,                        zero yes, tally yes
Tolerances are the grouped thermostat's own: positions 1e-9 A, each tally 1e-9 eV; held atoms bit for bit."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from firerig import BIG
from refloops import worse
import bathsref
import langevinref
import mdref
import oracle_bindings as ob

pytestmark = pytest.mark.gpu

GBIT = bathsref.INTEGRATE_BIT
BITS = bathsref.BATH_BITS
SKIN = 0.5
NSTEPS = 200
EVERY20 = tuple(range(20, 201, 20))
EVERY_ODD = (7, 14, 21, 49, 98, 133, 140, 161, 200)
BATHS = (dict(t_start=300.0, t_stop=900.0, damp=0.05, seed=48271, ratio={1: 2.0, 2: 0.5}, zero=True, tally=True),
         dict(t_start=100.0, t_stop=100.0, damp=0.02, seed=7919, ratio=None, zero=False, tally=True),
         dict(t_start=600.0, t_stop=200.0, damp=0.1, seed=48271, ratio=None, zero=True, tally=False))
BITS4 = bathsref.BATH_BITS4
BATHS4 = BATHS + (dict(t_start=200.0, t_stop=500.0, damp=0.03, seed=104729, ratio=None, zero=True, tally=True),)


def _system(style):
    if style == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
        return s, S.gaussian_velocities(s, 300.0, seed=91)
    af = capi.AeamFile(POT_AEAM)
    s = S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)
    s.mass[1:3] = af.mass[:2]
    return s, S.gaussian_velocities(s, 300.0, seed=93)


def _oracle_engine(oracle, style):
    if style == "rebomos":
        P = oracle.rebomos_params(POT_REBOMOS)
        return (lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)), 50
    T = oracle.aeam_pot(POT_AEAM)
    return (lambda sy: mdref.AeamCPU(oracle, T, sy, skin=1.0)), 25


def _context(style):
    ctx = capi.Context(0)
    if style == "rebomos":
        p = capi.read_rebomos_file(POT_REBOMOS)
        ctx.rebomos_set_params(p)
        return ctx, capi.STYLE_REBOMOS, 3.0 * p.rcmax[0][0] + SKIN, SKIN, [0, 0, 1]
    af = capi.AeamFile(POT_AEAM)
    tabs = af.build()
    ctx.aeam_set_tables(tabs)
    return ctx, capi.STYLE_AEAM, float(af.cut_table(tabs).max()) + SKIN, SKIN, None


def _ref_bath(s, b):
    return langevinref.Langevin(b["t_start"], b["t_stop"], b["damp"], b["seed"], s.mass, 0.001, S.FTM2V, boltz=S.BOLTZ, mvv2e=S.MVV2E,
                                ratio=b["ratio"], zero=b["zero"], tally=b["tally"])


def _dev_bath(b, bit, group):
    return dict(b, bit=bit, natoms=int(group.sum()))


def _case(style):
    s, v0 = _system(style)
    by_tag, g, groups = bathsref.masks(s)
    bathsref.check_masks(s, g, groups)                     # (conditions on the input, before anything is launched)
    assert np.all(np.abs(v0[~g]).max(axis=1) > 0.0)        # the held atoms are handed non-zero velocities
    return s, v0, by_tag, g, groups, S.wrap(s.box, s.x)


_REF = {}


def _reference(oracle, style):
    """the host loop of the three baths, once per style, read at both step sets"""
    if style not in _REF:
        s, v0 = _system(style)
        by_tag, g, groups = bathsref.masks(s)
        make, rebuild_every = _oracle_engine(oracle, style)
        baths = [(_ref_bath(s, b), l) for b, l in zip(BATHS, groups)]
        _REF[style] = bathsref.host_baths(make, s, v0, NSTEPS, set(EVERY20) | set(EVERY_ODD), rebuild_every, g, baths)
    return _REF[style]


def _by_tag(ctx, d, s):
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
    x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
    return x, v


def _layout(tags_local, by_tag, BITS=BITS):
    """what the device's atom order offers the kernels: (a 64-atom wave with atoms of all the baths, an unthermostatted
    and a held atom; a 256-atom block without a bath atom)"""
    m = by_tag[tags_local]
    anyb = sum(BITS)
    wave = block = False
    for i in range(0, len(m), 64):
        w = m[i:i + 64]
        wave = wave or (all(((w & b) != 0).any() for b in BITS) and (((w & GBIT) != 0) & ((w & anyb) == 0)).any()
                        and ((w & GBIT) == 0).any())
    for i in range(0, len(m) - 255, 256):
        block = block or not (m[i:i + 256] & anyb).any()
    return wave, block


def _resident(style, s, v0, by_tag, setup, ntally, every, nsteps=NSTEPS, check_layout=False, bits=BITS):
    """one resident brick; setup(d) sets the groups and the thermostat(s) (first = 0, last = nsteps).  Reads at `every`: a
    multiple of 14 among them finds its final half deferred (the tally read completes it), the others run it on their own.
    {step: (x, [tally of bath k], v)} by tag, and the device reneighborings while it ran"""
    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        setup(d)
        if check_layout:
            wave, block = _layout(d.tags_local, by_tag, bits)
            assert wave, f"no 64-atom wave holds all {len(bits)} baths, an unthermostatted and a held atom"
            assert block or len(bits) > 3, "no 256-atom block is free of bath atoms"     # (the fourth bath reaches into the left half)
        d.compute(1, 0)
        r0 = ctx.dd_info()["reneighbors"]
        out = {}
        for step in range(1, nsteps + 1):
            ev = step in every
            d.step(1 if ev else 0, 0, rebuild="auto", defer_final=(not ev) or step % 14 == 0)
            if ev:
                e = [d.langevin_tally(bath=k) for k in range(ntally)] if ntally else [d.langevin_tally()]
                d.flush()
                x, v = _by_tag(ctx, d, s)
                out[step] = (x, e, v)
        return out, ctx.dd_info()["reneighbors"] - r0
    finally:
        ctx.close()


def _three(by_tag, groups, order=(0, 1, 2), nsteps=NSTEPS):
    def setup(d):
        d.set_group(by_tag, GBIT)
        d.langevin_baths([_dev_bath(BATHS[k], BITS[k], groups[k]) for k in order], first=0, last=nsteps)
    return setup


def _compare(s, host, dev, g, x_in, v_in, what, every, xtol=1e-9, etol=1e-9):
    nb = len(next(iter(host.values()))[1])
    worst_x, worst_e = 0.0, [0.0] * nb
    for step in every:
        xh, eh, vh = host[step]
        xd, ed, vd = dev[step]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        worst_x = worse(worst_x, float(np.abs(dx).max()))
        assert len(ed) == len(eh) == nb
        for k in range(nb):
            worst_e[k] = worse(worst_e[k], abs(ed[k] - eh[k]))
        assert np.array_equal(xd[~g], x_in[~g]), (what, step, "a held atom moved")
        assert np.array_equal(vd[~g], v_in[~g]), (what, step, "a held atom's velocity changed")
    print(f"{what}: worst |dx| {worst_x:.2e} A, worst |dE| per bath {' '.join(f'{e:.2e}' for e in worst_e)} eV over {len(every)} reads")
    assert worst_x < xtol, worst_x
    assert max(worst_e) < etol, worst_e


_DEV = {}


def _three_baths_run(style, every):
    """the device run of case 1, kept for the cases that compare against it"""
    key = (style, every)
    if key not in _DEV:
        s, v0, by_tag, g, groups, x_in = _case(style)
        _DEV[key] = _resident(style, s, v0, by_tag, _three(by_tag, groups), 3, every, check_layout=True)
    return _DEV[key]


# ---- 1. resident, both styles, both step sets ---------------------------------------------------------------------
@pytest.mark.parametrize("every", [EVERY20, EVERY_ODD], ids=["every20", "odd"])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_three_baths_follow_the_host_reference(oracle, style, every, capsys):
    s, v0, by_tag, g, groups, x_in = _case(style)
    host = _reference(oracle, style)
    dev, renb = _three_baths_run(style, every)
    assert renb >= 1, "the device never reneighbored: the mask was not permuted"
    with capsys.disabled():
        _compare(s, host, dev, g, x_in, v0, f"three baths {style} ({[int(l.sum()) for l in groups]} of {int(g.sum())} group atoms, "
                 f"{renb} reneighborings)", every)
    last = host[NSTEPS][1]
    assert abs(last[0]) > 1e-3 and abs(last[1]) > 1e-3 and last[2] == 0.0 and dev[NSTEPS][1][2] == 0.0


def test_the_summed_tally_is_the_sum_in_bath_order():
    s, v0, by_tag, g, groups, x_in = _case("rebomos")
    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _three(by_tag, groups)(d)
        d.compute(1, 0)
        for step in range(1, NSTEPS + 1):
            d.step(0, 0, rebuild="auto", defer_final=True)
        e = [d.langevin_tally(bath=k) for k in range(3)]
        assert d.langevin_tally() == (e[0] + e[1]) + e[2] and e[0] != 0.0 and e[1] != 0.0 and e[2] == 0.0
    finally:
        ctx.close()


# ---- 2. one bath through langevin_baths is the one thermostat ---------------------------------------------------------
def test_one_bath_is_the_one_thermostat_bit_for_bit():
    s, v0, by_tag, g, groups, x_in = _case("rebomos")
    b, l = BATHS[0], groups[0]

    def through_baths(d):     # (the bath first: set_group without a langevin_bit leaves the one bath's bit in place)
        d.langevin_baths([_dev_bath(b, BITS[0], l)], first=0, last=NSTEPS)
        d.set_group(by_tag, GBIT)

    def as_before(d):
        d.set_group(by_tag, GBIT, BITS[0])
        d.langevin(b["t_start"], b["t_stop"], b["damp"], b["seed"], ratio=b["ratio"], zero=b["zero"], tally=b["tally"], first=0,
                   last=NSTEPS, natoms=int(l.sum()))
    new, renb = _resident("rebomos", s, v0, by_tag, through_baths, 1, EVERY_ODD)
    old, _ = _resident("rebomos", s, v0, by_tag, as_before, 0, EVERY_ODD)
    assert renb >= 1
    for step in EVERY_ODD:
        assert np.array_equal(new[step][0], old[step][0]) and np.array_equal(new[step][2], old[step][2]), step
        assert new[step][1] == old[step][1] and new[step][1][0] != 0.0, step


# ---- 3. a bath split in two ---------------------------------------------------------------------------------------
def test_a_split_bath_is_the_same_trajectory(capsys):
    """one `zero no tally yes` bath on L (bit 4) against two baths with the same numbers on the even and the odd tags of L
    (bits 8 and 16): the noise of an atom hangs on its tag alone, so x and v are equal bit for bit -- the many-bath kernels
    round as the one-bath kernels do --, and the two tallies add up to the one (1e-9 eV: other partial sums)"""
    s, v0, by_tag, g, groups, x_in = _case("rebomos")
    L = groups[0] | groups[1]
    b = dict(BATHS[1], t_start=300.0, t_stop=700.0)
    m = np.zeros_like(by_tag)
    m[s.tag] = 1 | np.where(g, GBIT, 0) | np.where(L, 4, 0) | np.where(L & (s.tag % 2 == 0), 8, 0) | np.where(L & (s.tag % 2 == 1), 16, 0)
    even, odd = L & (s.tag % 2 == 0), L & (s.tag % 2 == 1)
    assert even.sum() > 50 and odd.sum() > 50

    def one(d):
        d.set_group(m, GBIT)
        d.langevin_baths([_dev_bath(b, 4, L)], first=0, last=NSTEPS)

    def two(d):
        d.set_group(m, GBIT)
        d.langevin_baths([_dev_bath(b, 8, even), _dev_bath(b, 16, odd)], first=0, last=NSTEPS)
    a, renb = _resident("rebomos", s, v0, m, one, 1, EVERY_ODD)
    c, _ = _resident("rebomos", s, v0, m, two, 2, EVERY_ODD)
    assert renb >= 1
    worst = 0.0
    for step in EVERY_ODD:
        assert np.array_equal(a[step][0], c[step][0]) and np.array_equal(a[step][2], c[step][2]), step
        worst = worse(worst, abs(c[step][1][0] + c[step][1][1] - a[step][1][0]))
    with capsys.disabled():
        print(f"split bath: tally {a[NSTEPS][1][0]:.6f} eV = {c[NSTEPS][1][0]:.6f} + {c[NSTEPS][1][1]:.6f}, worst difference {worst:.2e} eV")
    assert abs(a[NSTEPS][1][0]) > 1e-3 and c[NSTEPS][1][0] != 0.0 and c[NSTEPS][1][1] != 0.0
    assert worst < 1e-9, worst


# ---- 4. the order of the bath slots; 5. reproducibility ---------------------------------------------------------------
def test_the_order_of_the_slots_changes_nothing():
    s, v0, by_tag, g, groups, x_in = _case("rebomos")
    a, _ = _three_baths_run("rebomos", EVERY_ODD)
    order = (2, 0, 1)
    b, renb = _resident("rebomos", s, v0, by_tag, _three(by_tag, groups, order), 3, EVERY_ODD)
    assert renb >= 1
    for step in EVERY_ODD:
        assert np.array_equal(a[step][0], b[step][0]) and np.array_equal(a[step][2], b[step][2]), step
        for slot, k in enumerate(order):
            assert b[step][1][slot] == a[step][1][k], (step, k)


# ---- 4b. the fourth slot: four baths against the reference, and every bath in slot 3 once --------------------------------
def _case4(style):
    s, v0 = _system(style)
    by_tag, g, groups = bathsref.masks4(s)
    bathsref.check_masks(s, g, groups)
    return s, v0, by_tag, g, groups, S.wrap(s.box, s.x)


def _four(by_tag, groups, order=(0, 1, 2, 3), nsteps=NSTEPS):
    def setup(d):
        d.set_group(by_tag, GBIT)
        d.langevin_baths([_dev_bath(BATHS4[k], BITS4[k], groups[k]) for k in order], first=0, last=nsteps)
    return setup


def _four_baths_run(style):
    key = (style, "four")
    if key not in _DEV:
        s, v0, by_tag, g, groups, x_in = _case4(style)
        _DEV[key] = _resident(style, s, v0, by_tag, _four(by_tag, groups), 4, EVERY_ODD, check_layout=True, bits=BITS4)
    return _DEV[key]


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_four_baths_follow_the_host_reference(oracle, style, capsys):
    """the fourth select of mdp_lgv_bath and the fourth tally slot: own ramp, damp, seed and tally per bath, `zero yes` on
    the fourth (its mean is taken over D's atoms alone).  The bounds of the three-bath cases"""
    s, v0, by_tag, g, groups, x_in = _case4(style)
    make, rebuild_every = _oracle_engine(oracle, style)
    baths = [(_ref_bath(s, b), l) for b, l in zip(BATHS4, groups)]
    host = bathsref.host_baths(make, s, v0, NSTEPS, set(EVERY_ODD), rebuild_every, g, baths)
    dev, renb = _four_baths_run(style)
    assert renb >= 1, "the device never reneighbored: the mask was not permuted"
    with capsys.disabled():
        _compare(s, host, dev, g, x_in, v0, f"four baths {style} ({[int(l.sum()) for l in groups]} of {int(g.sum())} group atoms, "
                 f"{renb} reneighborings)", EVERY_ODD)
    last = host[NSTEPS][1]
    assert abs(last[0]) > 1e-3 and abs(last[1]) > 1e-3 and last[2] == 0.0 and abs(last[3]) > 1e-3 and dev[NSTEPS][1][2] == 0.0
    # D's atoms are thermostatted: the run differs from the three-bath run on them
    three, _ = _three_baths_run(style, EVERY_ODD)
    assert np.abs(dev[NSTEPS][2][groups[3]] - three[NSTEPS][2][groups[3]]).max() > 1e-3


def test_the_order_of_four_slots_changes_nothing():
    """the three rotations of (A, B, C, D): with the run in order, every bath sits in slot 3 -- and in every other slot -- once"""
    s, v0, by_tag, g, groups, x_in = _case4("rebomos")
    a, _ = _four_baths_run("rebomos")
    for order in ((1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2)):
        b, renb = _resident("rebomos", s, v0, by_tag, _four(by_tag, groups, order), 4, EVERY_ODD)
        assert renb >= 1
        for step in EVERY_ODD:
            assert np.array_equal(a[step][0], b[step][0]) and np.array_equal(a[step][2], b[step][2]), (order, step)
            for slot, k in enumerate(order):
                assert b[step][1][slot] == a[step][1][k], (order, step, k)
    assert all(a[NSTEPS][1][k] != 0.0 for k in (0, 1, 3))


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_two_runs_of_the_three_baths_agree(style, capsys):
    """REBO-MoS: bit for bit, tallies included -- its forces and the baths' sums are added in a fixed order.  The alloy's
    three-body forces use float atomics, so its runs agree to rounding with or without a thermostat: two runs are held to
    1e-12 A, 1e-11 A/ps and 1e-12 eV per tally -- a force that differs in its last bits (1e-16 relative) grows by the
    lattice's Lyapunov rate of a few per ps to well below that in 0.2 ps, while a bath sum taken in another order every
    run would move a tally of some eV in its 1e-16 relative too, and a wrong bath on one atom by far more"""
    s, v0, by_tag, g, groups, x_in = _case(style)
    wx = wv = we = 0.0
    for every in (EVERY20, EVERY_ODD):
        a, _ = _three_baths_run(style, every)
        b, _ = _resident(style, s, v0, by_tag, _three(by_tag, groups), 3, every)
        for step in every:
            if style == "rebomos":
                assert np.array_equal(a[step][0], b[step][0]) and np.array_equal(a[step][2], b[step][2]), step
                assert a[step][1] == b[step][1], step
            wx = worse(wx, float(np.abs(a[step][0] - b[step][0]).max()))
            wv = worse(wv, float(np.abs(a[step][2] - b[step][2]).max()))
            we = worse(we, max(abs(p - q) for p, q in zip(a[step][1], b[step][1])))
    with capsys.disabled():
        print(f"two runs of the three baths, {style}: |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps, |dE| {we:.2e} eV")
    assert wx < 1e-12 and wv < 1e-11 and we < 1e-12, (wx, wv, we)


# ---- 6. host-linked mode from shuffled atoms ----------------------------------------------------------------------------
def _hostlinked(oracle, style, s, v0, x_in, by_tag, g, baths, every, refused=None):
    """mdp_hnve_* with mdp_hnve_set_mask and `baths` (dicts of _dev_bath): the host's atom order is a shuffle of the tags, host
    reneighborings every 50 steps re-upload atoms, velocities and mask (each upload counts the atoms in more than one
    bath again).  The alloy on the library's own lists, as under the plugin; REBO-MoS in the device's own order, so the mask,
    tags and types are read through the host's permutation.  refused: what an initial half without a mask must answer.
    {step: (x, [tally of bath k], v)} by tag at `every`, and the uploads"""
    import ctypes as C
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
        c.hnve_setup(0.001, S.FTM2V, s.mass)
        c.integrate_group(GBIT)
        cfgs = []
        for b in baths:
            b = dict(b)
            b["t_period"] = b.pop("damp")
            cfgs.append(b)
        c.langevin_baths(cfgs, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        c.langevin_run(0, NSTEPS)
        upload(x_in[perm].copy(), v0[perm])
        assert c.host_ghosts_derived()
        if refused:
            with pytest.raises(capi.MdpError, match=refused):
                c.hnve_initial()
        c.hnve_set_mask(mask_p)
        compute()
        dev, uploads = {}, 0
        for step in range(1, NSTEPS + 1):
            moved, late = c.hnve_initial()
            if moved or step % 50 == 0:     # the host's reneighboring: atoms come up, are wrapped and go down again, mask included
                got = c.hnve_download(s.n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]     # (a host that wraps rewrites only atoms that left the box: the held ones did not)
                upload(xw, got["v"])
                c.hnve_set_mask(mask_p)
                uploads += 1
            compute()
            c.hnve_final()
            if step in every:
                e = [c.langevin_tally(bath=k) for k in range(len(cfgs))]
                got = c.hnve_download(s.n, want=("x", "v"))
                xd, vd = np.zeros((s.n, 3)), np.zeros((s.n, 3))
                xd[tag_p - 1], vd[tag_p - 1] = got["x"], got["v"]
                dev[step] = (xd, e, vd)
    finally:
        c.close()
    return dev, uploads


@pytest.mark.parametrize("style", ["aeam", "rebomos"])
def test_hostlinked_baths_from_shuffled_atoms(oracle, style, capsys):
    """the three baths through _hostlinked against the host loop; before the mask is there an initial half is refused"""
    s, v0, by_tag, g, groups, x_in = _case(style)
    host = _reference(oracle, style)
    dev, uploads = _hostlinked(oracle, style, s, v0, x_in, by_tag, g, [_dev_bath(BATHS[k], BITS[k], groups[k]) for k in range(3)],
                               EVERY20, refused="3 Langevin baths are on .* but no mask covers the current atoms")
    assert uploads >= 3
    with capsys.disabled():
        _compare(s, host, dev, g, x_in, v0, f"three baths, host-linked {style}, shuffled host order ({uploads} uploads)", EVERY20)


def test_hostlinked_split_bath_is_the_same_trajectory(oracle, capsys):
    """test_a_split_bath_is_the_same_trajectory through mdp_hnve_initial / mdp_hnve_final from shuffled atoms: the one bath
    runs the NB = 1 kernels with tags, types and mask read through the host's permutation, the two baths the NB = 4 kernels
    -- both from the same templates.  x and v equal bit for bit at every read, the two tallies add up to the one (1e-9 eV)"""
    s, v0, by_tag, g, groups, x_in = _case("rebomos")
    L = groups[0] | groups[1]
    b = dict(BATHS[1], t_start=300.0, t_stop=700.0)
    even, odd = L & (s.tag % 2 == 0), L & (s.tag % 2 == 1)
    m = np.zeros_like(by_tag)
    m[s.tag] = 1 | np.where(g, GBIT, 0) | np.where(L, 4, 0) | np.where(even, 8, 0) | np.where(odd, 16, 0)
    assert even.sum() > 50 and odd.sum() > 50
    a, uploads = _hostlinked(oracle, "rebomos", s, v0, x_in, m, g, [_dev_bath(b, 4, L)], EVERY20)
    c, _ = _hostlinked(oracle, "rebomos", s, v0, x_in, m, g, [_dev_bath(b, 8, even), _dev_bath(b, 16, odd)], EVERY20)
    assert uploads >= 3
    worst = 0.0
    for step in EVERY20:
        assert np.array_equal(a[step][0], c[step][0]) and np.array_equal(a[step][2], c[step][2]), step
        worst = worse(worst, abs(c[step][1][0] + c[step][1][1] - a[step][1][0]))
    with capsys.disabled():
        print(f"host-linked split bath: tally {a[NSTEPS][1][0]:.6f} eV = {c[NSTEPS][1][0]:.6f} + {c[NSTEPS][1][1]:.6f}, "
              f"worst difference {worst:.2e} eV")
    assert abs(a[NSTEPS][1][0]) > 1e-3 and c[NSTEPS][1][0] != 0.0 and c[NSTEPS][1][1] != 0.0
    assert worst < 1e-9, worst


# ---- 6b. more than 256 per-block partials with two baths --------------------------------------------------------------------
@pytest.mark.parametrize("style", ["aeam", "rebomos"])
def test_two_baths_sum_every_partial(style, capsys):
    """test_gpu_langevin_mdp.test_zero_and_tally_sum_every_partial with two baths, on the even and on the odd tags of the same
    cell: more than 256 per-block partials, so mdp_slot_sum_256 makes a second trip with the 12 values per slot of the
    means and the 4 of the tallies.  Both baths zero yes and tally yes, seeds, damping and ramps of their own, a ratio on
    the first.  Per step the written-back force of every atom must be langevinref's for ITS bath, with that bath's mean of
    the random parts taken by math.fsum over that bath's atoms, to 1e-12 eV/A; each bath's tally must be
    -(e_0 / 2 + e_1 + ... + e_k / 2) dt with e = fsum(f_L . v) over its atoms, to 1e-12 of its scale (the bounds and their
    reasons are that test's)"""
    import math
    import test_gpu_langevin_mdp as LM
    import test_gpu_nvt_net as NN
    s, v0 = NN._big(style)
    assert s.n > 65536 and -(-s.n // 256) > 256
    dt, nsteps, bits = 0.001, 3, (8, 16)
    spec = (dict(t_start=300.0, t_stop=330.0, damp=0.05, seed=48271, ratio={1: 2.0, 2: 0.5}, zero=True, tally=True),
            dict(t_start=250.0, t_stop=200.0, damp=0.02, seed=7919, ratio=None, zero=True, tally=True))
    lgs = [_ref_bath(s, b) for b in spec]
    for lg in lgs:
        lg.setup(0, nsteps)
    by_tag = np.zeros(int(s.tag.max()) + 1, dtype=np.int32)
    by_tag[s.tag] = 1 | np.where(s.tag % 2 == 0, bits[0], bits[1])
    count = [int((s.tag % 2 == 0).sum()), int((s.tag % 2 == 1).sum())]
    dtf = 0.5 * dt * S.FTM2V
    ctx, d = LM._domain(capi.STYLE_AEAM if style == "aeam" else capi.STYLE_REBOMOS, s, v0)

    def f_l(step, tags, types, v, phase=0):
        out = np.zeros_like(v)
        for k, lg in enumerate(lgs):
            sel = tags % 2 == k
            fran = lg.random(step, tags[sel], types[sel], phase)
            mean = np.array([math.fsum(fran[:, j]) for j in range(3)]) / count[k]
            out[sel] = lg.g1[types[sel]][:, None] * v[sel] + fran - mean
        return out

    def dots(a, b, tags):
        p = a * b
        return [(math.fsum(p[tags % 2 == k].ravel()), math.fsum(np.abs(p[tags % 2 == k]).ravel())) for k in range(2)]
    try:
        d.set_group(by_tag, 0)
        d.langevin_baths([dict(b, bit=bits[k], natoms=count[k]) for k, b in enumerate(spec)], first=0, last=nsteps)
        d.compute(0, 0)
        tags, types = d.tags_local.copy(), ctx.md_download_int("type", d.nlocal).copy()
        assert (tags % 2 == 0).sum() == count[0]
        m = s.mass[types][:, None]
        worst_f, worst_e = 0.0, [0.0, 0.0]
        # the setup force: in the first initial half
        a = ctx.md_download(d.nlocal, want=("v", "f"))
        ctx.md_initial_integrate()
        b = ctx.md_download(d.nlocal, want=("v",))
        want = f_l(0, tags, types, a["v"], phase=1)
        assert np.abs(a["f"]).max() < 100.0
        worst_f = worse(worst_f, float(np.abs((b["v"] - a["v"]) * m / dtf - a["f"] - want).max()))
        acc = [dict(energy=0.5 * e * dt, e_last=e, scale=0.5 * sc * dt) for e, sc in dots(want, a["v"], tags)]
        for step in range(1, nsteps + 1):
            if step > 1:
                ctx.md_initial_integrate()
            ctx.md_compute(0, 0)
            assert np.array_equal(d.tags_local, tags)            # (no reneighbouring in three steps: same slots)
            a = ctx.md_download(d.nlocal, want=("v", "f"))
            ctx.md_final_integrate()
            b = ctx.md_download(d.nlocal, want=("v", "f"))
            want = f_l(step, tags, types, a["v"])
            assert np.abs(a["f"]).max() < 100.0
            worst_f = worse(worst_f, float(np.abs(b["f"] - a["f"] - want).max()))
            for k, (e, ea) in enumerate(dots(want, b["v"], tags)):
                t = acc[k]
                t.update(energy=t["energy"] + e * dt, e_last=e, scale=t["scale"] + ea * dt)
                got = ctx.langevin_tally(bath=k)
                worst_e[k] = worse(worst_e[k], abs(got + (t["energy"] - 0.5 * t["e_last"] * dt)) / t["scale"])
            assert np.abs(b["v"] - a["v"] - dtf * b["f"] / m).max() < 1e-12   # and the final half used f + f_L
    finally:
        ctx.close()
    with capsys.disabled():
        print(f"{style} {s.n} atoms, two baths: worst |f_L - reference| {worst_f:.2e} eV/A, tallies {worst_e[0]:.2e} and {worst_e[1]:.2e} "
              f"of their scales")
    assert worst_f < 1e-12, worst_f
    assert max(worst_e) < 1e-12, worst_e


# ---- 7. bricks ----------------------------------------------------------------------------------------------------
def _bricks(style, s, v0, by_tag, groups, world, nsteps=NSTEPS, renb=5):
    """the three baths without zero / tally (they need one rank) on `world` resident bricks, list builds forced every `renb`
    steps; x, v by tag at the end, atoms that changed owner, whether the mask came back"""
    def rank_fn(r, make_tr):
        ctx, st, cutghost, skin, map_ = _context(style)
        try:
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=make_tr(ctx) if world > 1 else None)
            d.set_group(by_tag, GBIT)
            d.langevin_baths([_dev_bath(dict(BATHS[k], zero=False, tally=False), BITS[k], groups[k]) for k in range(3)], first=0,
                             last=nsteps)
            d.compute(1, 0)
            left = 0
            for step in range(1, nsteps + 1):
                rb = step % renb == 0
                d.step(0, 0, rebuild=rb, defer_final=step < nsteps)
                if rb:
                    left += ctx.dd_info()["left_last"]
            d.flush()
            got = ctx.md_download(d.nlocal, want=("x", "v"))
            return dict(tags=d.tags_local.copy(), x=got["x"], v=got["v"], mask=d.mask_local().copy(), left=left)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    x, v, seen = np.zeros((s.n, 3)), np.zeros((s.n, 3)), np.zeros(s.n, dtype=int)
    mask_ok = True
    for r in res:
        x[r["tags"] - 1], v[r["tags"] - 1] = r["x"], r["v"]
        seen[r["tags"] - 1] += 1
        mask_ok = mask_ok and np.array_equal(r["mask"], by_tag[r["tags"]])
    assert np.all(seen == 1)
    return x, v, sum(r["left"] for r in res), mask_ok


_ONE = {}


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_bricks_carry_the_baths_through_migration(style, world, capsys):
    """the trajectory by tag of 2 and 4 bricks equals the one-rank run to the bound of the multi-rank Langevin test (1e-8 A,
    1e-7 A/ps); the bath atoms drift (-15, -12, -9 A/ps on top of 300 K) so that atoms change owner, each with its mask and
    so with its bath"""
    s, v0, by_tag, g, groups, x_in = _case(style)
    v0 = v0.copy()
    v0[groups[0] | groups[1] | groups[2]] += np.array([-15.0, -12.0, -9.0])
    if style not in _ONE:
        _ONE[style] = _bricks(style, s, v0, by_tag, groups, 1)
    x1, v1, _, ok1 = _ONE[style]
    xn, vn, left, okn = _bricks(style, s, v0, by_tag, groups, world)
    assert left >= 1, "no atom changed owner: no bath atom migrated"
    assert ok1 and okn
    dx = xn - x1
    dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
    wx, wv = float(np.abs(dx).max()), float(np.abs(vn - v1).max())
    with capsys.disabled():
        print(f"bath bricks {style} x {world}: {left} atoms changed owner, |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps against one rank")
    assert wx < 1e-8 and wv < 1e-7
    assert np.array_equal(xn[~g], x_in[~g]) and np.array_equal(vn[~g], v0[~g])


# ---- 8. refusals, and langevin_off ----------------------------------------------------------------------------------------
def _cfg(k=0, bit=None, natoms=100, **kw):
    b = dict(BATHS[k], bit=BITS[k] if bit is None else bit, natoms=natoms)
    b["t_period"] = b.pop("damp")
    b.update(kw)
    return b


def test_library_refusals():
    s, v0, by_tag, g, groups, x_in = _case("rebomos")
    c = capi.Context(0)
    try:
        # the number of baths, their bits, their numbers
        with pytest.raises(capi.MdpError, match="0 baths; a context takes 1 to 4") as e:
            c.langevin_baths([])
        assert e.value.code == -1                           # MDP_EINVAL
        with pytest.raises(capi.MdpError, match="5 baths; a context takes 1 to 4"):
            c.langevin_baths([_cfg(0, bit=4 << k) for k in range(5)])
        with pytest.raises(capi.MdpError, match="bath 1 has group bit 0"):
            c.langevin_baths([_cfg(0), _cfg(1, bit=0)])
        with pytest.raises(capi.MdpError, match="bath 0 has group bit 0"):
            c.langevin_baths([_cfg(0, bit=0)])
        with pytest.raises(capi.MdpError, match="baths 0 and 2 share the group bit 4"):
            c.langevin_baths([_cfg(0), _cfg(1), _cfg(2, bit=4)])
        for kw, what in ((dict(seed=0), "bath 1: the seed must be > 0"), (dict(t_period=0.0), "bath 1: damp must be > 0"),
                         (dict(t_start=-1.0), "bath 1: Tstart and Tstop must be >= 0"), (dict(t_stop=-5.0), "bath 1: Tstart and Tstop"),
                         (dict(ratio={2: 0.0}), "bath 1: the scale ratio of type 2 must be > 0"),
                         (dict(zero=True, natoms=0), "bath 1: boltz, mvv2e or natoms out of range")):
            with pytest.raises(capi.MdpError, match=what):
                c.langevin_baths([_cfg(0), _cfg(1, **kw)])
        with pytest.raises(capi.MdpError, match="mdp_langevin_setup not called"):
            c.langevin_tally(bath=0)                        # nothing above switched a thermostat on
        # a Nose-Hoover chain, in either order
        c.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_langevin_baths: the Nose-Hoover chain"):
            c.langevin_baths([_cfg(0), _cfg(1)])
        c.nhc_off()
        c.langevin_baths([_cfg(0), _cfg(1)])
        with pytest.raises(capi.MdpError, match="mdp_nhc_setup: the Langevin thermostat"):
            c.nhc_setup(300.0, 300.0, 0.1, 30.0)
        # the group call of the one thermostat, and a bath index
        with pytest.raises(capi.MdpError, match="mdp_langevin_group: 2 Langevin baths are on"):
            c.langevin_group(4)
        with pytest.raises(capi.MdpError, match="bath index 2 out of range"):
            c.langevin_tally(bath=2)
        with pytest.raises(capi.MdpError, match="bath index -1 out of range"):
            c.langevin_tally(bath=-1)
        c.langevin_baths([_cfg(0)])                         # one bath: the one thermostat, its group call is back
        c.langevin_group(0)
        with pytest.raises(capi.MdpError, match="bath index 1 out of range"):
            c.langevin_tally(bath=1)
        c.langevin_off()
    finally:
        c.close()

    # on a resident brick: no mask, overlapping groups (counted on the device), a minimisation in either order
    D = lambda k: _dev_bath(BATHS[k], BITS[k], groups[k])   # noqa: E731
    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0.copy())
        d.compute(1, 0)
        d.langevin_baths([D(0), D(1)], first=0, last=10)
        with pytest.raises(capi.MdpError, match="2 Langevin baths are on .* but no mask covers the current atoms") as e:
            ctx.md_initial_integrate()
        assert e.value.code == -6                           # MDP_ESTATE
        over = by_tag.copy()
        both = groups[0] & (s.tag % 8 == 0)
        over[s.tag[both]] |= BITS[1]
        n_over = int(both.sum())
        assert n_over > 5
        with pytest.raises(capi.MdpError, match=f"mdp_md_set_mask: {n_over} atoms are in more than one of the 2 Langevin baths"):
            d.set_group(over, GBIT)
        with pytest.raises(capi.MdpError, match=f"{n_over} atoms are in more than one"):
            ctx.md_initial_integrate()                      # (the refused mask is on the device: nothing advances with it)
        d.langevin_off()
        d.set_group(over, GBIT)                             # (without baths any mask will do)
        with pytest.raises(capi.MdpError, match=f"mdp_langevin_baths: {n_over} atoms are in more than one of the 3 Langevin baths"):
            d.langevin_baths([D(0), D(1), D(2)])
        d.langevin_baths([D(0), D(2)])                      # (baths A and C of that mask are disjoint)
        d.set_group(by_tag, GBIT)
        d.langevin_baths([D(0), D(1), D(2)])
        with pytest.raises(ValueError, match="3 Langevin baths are on"):
            d.set_group(by_tag, GBIT, BITS[0])              # (each bath has the bit it was given)
        with pytest.raises(capi.MdpError, match="mdp_fire_setup: a thermostat"):
            ctx.fire_setup(0.0, 0.0, BIG, BIG)
        d.langevin_off()
        ctx.fire_setup(0.0, 0.0, BIG, BIG)
        with pytest.raises(capi.MdpError, match="mdp_langevin_baths: a minimisation"):
            d.langevin_baths([D(0), D(1)])
        ctx.fire_off()
    finally:
        ctx.close()

    # zero / tally in any bath on a brick of several ranks, in either order
    p = capi.read_rebomos_file(POT_REBOMOS)
    cutghost = 3.0 * p.rcmax[0][0] + 2.0
    plain = [_cfg(0, zero=False, tally=False), _cfg(1, zero=False, tally=False)]
    for kw in ({"zero": True}, {"tally": True}):
        for baths_first in (True, False):
            c = capi.Context(0)
            try:
                c.rebomos_set_params(p)
                resident.DeviceDomain(c, capi.STYLE_REBOMOS, s, cutghost, 2.0, [0, 0, 1], v0=v0.copy())
                sums = [plain[0], _cfg(1, **dict(dict(zero=False, tally=False), **kw))]
                if baths_first:
                    c.langevin_baths(sums)
                    with pytest.raises(capi.MdpError, match="one rank only"):
                        c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
                else:
                    c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
                    with pytest.raises(capi.MdpError, match="bath 1: zero and tally run on one rank only"):
                        c.langevin_baths(sums)
                    c.langevin_baths(plain)                 # (without them a brick takes the baths)
            finally:
                c.close()


def test_langevin_off_after_baths_gives_back_nve(capsys):
    """60 steps with the three baths, mdp_langevin_off, then 100 steps: the spread of the total energy stays within that of
    an NVE run on a fresh context from the same state (1e-6 eV on top: the two follow the same trajectory to rounding, and a
    bath still on would move the total by the 1e-2 eV per 100 steps its tally shows)"""
    s, v0, by_tag, g, groups, x_in = _case("rebomos")

    def spread(d):
        d.compute(1, 0)
        e = []
        for step in range(1, 101):
            d.step(1, 0, rebuild="auto", defer_final=False)
            t = d.thermo()
            e.append(t["ke"] + t["pe"])
        return max(e) - min(e)
    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _three(by_tag, groups, nsteps=60)(d)
        d.compute(1, 0)
        for step in range(1, 61):
            d.step(0, 0, rebuild="auto", defer_final=True)
        exchanged = abs(d.langevin_tally())
        d.langevin_off()
        with pytest.raises(capi.MdpError, match="mdp_langevin_setup not called"):
            ctx.langevin_tally(bath=0)
        x, v = _by_tag(ctx, d, s)
        after = spread(d)
    finally:
        ctx.close()
    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, S.System(s.box, S.wrap(s.box, x), s.type, s.tag, s.mass), cutghost, skin, map_, v0=v)
        d.set_group(by_tag, GBIT)
        nve = spread(d)
    finally:
        ctx.close()
    with capsys.disabled():
        print(f"after langevin_off: etotal spread {after:.3e} eV over 100 steps, NVE from the same state {nve:.3e} eV; the baths "
              f"had exchanged {exchanged:.3e} eV in 60 steps")
    assert exchanged > 1e-3
    assert after <= nve + 1e-6, (after, nve)
