"""GPU: constant-flux heat sources on groups (mdp_heat_setup / _run / _state / _off; heat_sums_kernel, heat_control_kernel
and heat_apply_kernel of csrc/heat.hip behind every final half) against the masked host loop of tests/heatref.py around the
ORACLE forces.

The two cells of the several-bath tests at 300 K, 200 steps of 0.001 ps with rebuild="auto" and a 0.5 A skin.  The masks are
bathsref.masks: bath A (bit 4) is the source, bath B (bit 8) the sink, bath C's atoms are plain integrated atoms, a third of
the cell is held.  B's atoms carry an extra drift of (0.5, -0.3, 0.2) A/ps, so that vsub = (scale - 1) vcm is exercised.
eflux_k = +-1e-3 KEcm_k(0) / dt.  Tolerances are the project's own for these cells and step counts under a global-sum
feedback: positions 1e-9 A (the grouped thermostats), velocities 2e-8 A/ps (VTOL of tests/test_gpu_langevin_mdp.py, the
one velocity bound those tests hold against a host loop), held atoms bit for bit, the scale 1e-12 relative.  The reference
with every source's atoms summed in a permuted order stays 100 times inside them (test_a_permuted_sum_..., no GPU).

The fixed cases above use two sources, one nevery, first = 0 and one run.  Section 6 holds what tests/nets.py's `heat` net
cannot carry: four sources with four different nevery from first = 7 with the state read at every step, two runs in a row on
one context (mdp_heat_run at a due step; resident with the seam's final half pending or completed, and host-linked), and
275 684 atoms -- 270 partial slots, the control workgroup's second trip -- against math.fsum."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from firerig import BIG
from refloops import worse
import bathsref
import heatref
import mdref
import nets
import oracle_bindings as ob

gpu = pytest.mark.gpu

GBIT = bathsref.INTEGRATE_BIT
SRC_BIT, SINK_BIT = bathsref.BATH_BITS[0], bathsref.BATH_BITS[1]
SKIN = 0.5
NSTEPS = 200
DT = 0.001
EVERY20 = tuple(range(20, 201, 20))
EVERY_ODD = (7, 14, 21, 49, 98, 133, 140, 161, 200)
DRIFT = np.array([0.5, -0.3, 0.2])
XTOL, VTOL, STOL = 1e-9, 2e-8, 1e-12


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


def _kecm(s, v, group):
    """the group's kinetic energy about its centre of mass, in energy units"""
    return heatref.kecm(v, s.mass[s.type], group, S.FTM2V, S.MVV2E) * S.MVV2E


_CASE = {}


def _case(style):
    """(system, v0 with the sink's drift, mask by tag, integrate group, [source, sink], wrapped positions, [eflux])"""
    if style not in _CASE:
        s, v0 = _system(style)
        by_tag, g, groups = bathsref.masks(s)
        bathsref.check_masks(s, g, groups)
        v0 = v0.copy()
        v0[groups[1]] += DRIFT
        assert np.all(np.abs(v0[~g]).max(axis=1) > 0.0)        # the held atoms are handed non-zero velocities
        flux = [1e-3 * _kecm(s, v0, groups[0]) / DT, -1e-3 * _kecm(s, v0, groups[1]) / DT]
        _CASE[style] = (s, v0, by_tag, g, groups[:2], S.wrap(s.box, s.x), flux)
    return _CASE[style]


def _ref_sources(style, nevery=1):
    s, v0, by_tag, g, groups, x_in, flux = _case(style)
    return [dict(group=groups[k], eflux=flux[k], nevery=nevery) for k in range(2)]


def _dev_sources(style, nevery=1, flux=None):
    f = _case(style)[6] if flux is None else flux
    return [dict(eflux=f[0], nevery=nevery, bit=SRC_BIT), dict(eflux=f[1], nevery=nevery, bit=SINK_BIT)]


_REF = {}


def _reference(oracle, style, nevery=1, permuted=False):
    """the host loop of the two sources, once per case, read at both step sets; every escale of it is > 0.5"""
    key = (style, nevery, permuted)
    if key not in _REF:
        s, v0, by_tag, g, groups, x_in, flux = _case(style)
        make, rebuild_every = _oracle_engine(oracle, style)
        orders = None
        if permuted:
            rng = np.random.default_rng(5)
            orders = [rng.permutation(int(l.sum())) for l in groups]
        out, lowest = heatref.host_heat(make, s, v0, NSTEPS, set(EVERY20) | set(EVERY_ODD), rebuild_every, g,
                                        _ref_sources(style, nevery), dt=DT, orders=orders)
        assert lowest > 0.5, lowest
        _REF[key] = out
    return _REF[key]


def _by_tag(ctx, d, s):
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
    x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
    return x, v


def _layout(tags_local, by_tag):
    """what the device's atom order offers the kernels: (a 64-atom wave with source, sink, plain and held atoms; a
    256-atom block without an atom of either source)"""
    m = by_tag[tags_local]
    both = SRC_BIT | SINK_BIT
    wave = block = False
    for i in range(0, len(m), 64):
        w = m[i:i + 64]
        wave = wave or (((w & SRC_BIT) != 0).any() and ((w & SINK_BIT) != 0).any()
                        and (((w & GBIT) != 0) & ((w & both) == 0)).any() and ((w & GBIT) == 0).any())
    for i in range(0, len(m) - 255, 256):
        block = block or not (m[i:i + 256] & both).any()
    return wave, block


def _resident(style, sources, every, nsteps=NSTEPS, defer="mixed", check_layout=False, first=0):
    """one resident brick with the integrate group and `sources` (None: plain NVE on the group).  Reads at `every`; with
    defer="mixed" a read at a multiple of 14 finds its final half deferred (the state read completes it, heat pass
    included), the others run it on their own; "all" / "none": every final half deferred / none.
    {step: (x, [scale of source k], v)} by tag, and the device reneighborings while it ran"""
    s, v0, by_tag, g, groups, x_in, flux = _case(style)
    ctx, st, cutghost, skin, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        if sources is not None:
            d.heat(sources, first=first)
        if check_layout:
            wave, block = _layout(d.tags_local, by_tag)
            assert wave, "no 64-atom wave holds source, sink, plain and held atoms"
            assert block, "no 256-atom block is free of source atoms"
        d.compute(1, 0)
        r0 = ctx.dd_info()["reneighbors"]
        out = {}
        for step in range(1, nsteps + 1):
            ev = step in every
            df = {"mixed": (not ev) or step % 14 == 0, "all": True, "none": False}[defer]
            d.step(0, 0, rebuild="auto", defer_final=df)
            if ev:
                sc = [d.heat_state(k)["scale"] for k in range(len(sources))] if sources is not None else []
                d.flush()
                x, v = _by_tag(ctx, d, s)
                out[step] = (x, sc, v)
        return out, ctx.dd_info()["reneighbors"] - r0
    finally:
        ctx.close()


def _compare(s, host, dev, g, x_in, v_in, what, every, scale=1.0):
    """`scale`: the fraction of the bounds the comparison is held to.  x_in=None: `dev` is a host loop too, whose rebuilds
    wrap the held atoms as well -- they are compared with the other loop's"""
    wx = wv = ws = 0.0
    for step in every:
        xh, sh, vh = host[step]
        xd, sd, vd = dev[step]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        wx = worse(wx, float(np.abs(dx).max()))
        wv = worse(wv, float(np.abs(vd - vh).max()))
        for a, b in zip(sd, sh):
            ws = worse(ws, abs(a - b) / abs(b))
        assert len(sd) == len(sh)
        assert np.array_equal(xd[~g], (xh if x_in is None else x_in)[~g]), (what, step, "a held atom moved")
        assert np.array_equal(vd[~g], v_in[~g]), (what, step, "a held atom's velocity changed")
    print(f"{what}: worst |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps, scale {ws:.2e} relative over {len(every)} reads")
    assert wx < XTOL * scale and wv < VTOL * scale and ws < STOL * scale, (wx, wv, ws)


_DEV = {}


def _two_sources_run(style, every):
    key = (style, every)
    if key not in _DEV:
        _DEV[key] = _resident(style, _dev_sources(style), every, check_layout=True)
    return _DEV[key]


# ---- 0. the reference itself, on the CPU: the order the group's atoms are summed in ------------------------------------
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_a_permuted_sum_stays_a_hundred_times_inside_the_bounds(oracle, style, capsys):
    """no GPU.  The device adds a group's atoms in its own order (per block, then the blocks); the reference run with every
    source's atoms added in a random order differs from the one in the order of the cell by 100 times less than the
    bounds the device is held to (the spread is in DESIGN.md section 5)"""
    s, v0, by_tag, g, groups, x_in, flux = _case(style)
    a, b = _reference(oracle, style), _reference(oracle, style, permuted=True)
    every = tuple(sorted(a))
    with capsys.disabled():
        _compare(s, a, b, g, None, v0, f"permuted sums {style}", every, scale=0.01)
    assert all(a[n][1][1] < 1.0 < a[n][1][0] for n in every)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heatref", "host_heat_fixed_cases.npz")


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_the_generalised_host_loop_gives_the_fixed_cases_bit_for_bit(oracle, style):
    """no GPU.  heatref.host_heat took first, dt, a cut, the skin assertion and the state words for the net; with none of
    them given it is the loop the fixed cases were merged with: the scales of all 17 reads and x, v of the last step,
    plain and with permuted sums, against a run saved from the loop before it was generalised.

    Where the file comes from: tests/heatref.py of commit 1696e2d ("Add fix heat/mdp: constant-flux heat sources on
    groups, on the device"), the loop as merged, put in place of today's; then, for both styles and permuted in (False,
    True), r = _reference(oracle, style, permuted=permuted) of this module (same cells, sources and arguments then as
    now) and np.savez_compressed(GOLDEN, ...) of, under key = f"{style}_{'permuted' if permuted else 'plain'}":
    key_steps = sorted(r), key_scales = [r[n][1] for n in steps], key_x = r[NSTEPS][0], key_v = r[NSTEPS][2].
    Repeating that reproduces every array of the file bit for bit.  The file changes only if the reference is MEANT to
    give other numbers for the fixed cases; anything else that breaks this test is a regression of the loop."""
    gold = np.load(GOLDEN)
    for permuted in (False, True):
        r = _reference(oracle, style, permuted=permuted)
        key = f"{style}_{'permuted' if permuted else 'plain'}"
        steps = sorted(r)
        assert steps == gold[key + "_steps"].tolist()
        assert np.array_equal(np.array([r[n][1] for n in steps]), gold[key + "_scales"]), key
        assert np.array_equal(r[NSTEPS][0], gold[key + "_x"]) and np.array_equal(r[NSTEPS][2], gold[key + "_v"]), key


# ---- 1. resident, both styles, both step sets ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("every", [EVERY20, EVERY_ODD], ids=["every20", "odd"])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_source_and_sink_follow_the_host_reference(oracle, style, every, capsys):
    s, v0, by_tag, g, groups, x_in, flux = _case(style)
    host = _reference(oracle, style)
    dev, renb = _two_sources_run(style, every)
    assert renb >= 1, "the device never reneighbored: the mask was not permuted"
    with capsys.disabled():
        _compare(s, host, dev, g, x_in, v0, f"source and sink {style} ({[int(l.sum()) for l in groups]} of {int(g.sum())} group atoms, "
                 f"{renb} reneighborings)", every)
    assert dev[NSTEPS][1][0] > 1.0 > dev[NSTEPS][1][1]      # the source heats, the sink cools


@gpu
def test_nevery_three_follows_the_host_reference(oracle, capsys):
    s, v0, by_tag, g, groups, x_in, flux = _case("rebomos")
    host = _reference(oracle, "rebomos", nevery=3)
    dev, renb = _resident("rebomos", _dev_sources("rebomos", nevery=3), EVERY_ODD)
    with capsys.disabled():
        _compare(s, host, dev, g, x_in, v0, "source and sink rebomos, nevery 3", EVERY_ODD)
    one = _reference(oracle, "rebomos")
    assert abs(host[7][1][0] - 1.0) > 2.0 * abs(one[7][1][0] - 1.0)    # (three steps' worth per application)


# ---- 2. no flux; deferred or not; twice ---------------------------------------------------------------------------------
@gpu
def test_sources_without_flux_are_the_plain_run_bit_for_bit():
    """escale = ((ke - t) + 0) / (ke - t) = 1, scale = 1, vsub = 0, v = fma(1, v, -0) = v; the plain run does not defer
    (with sources on the final and the initial half are never fused, and the fused kernel rounds its two kicks otherwise)"""
    every = (7, 49, 133, 200)
    a, renb = _resident("rebomos", _dev_sources("rebomos", flux=[0.0, 0.0]), every)
    b, _ = _resident("rebomos", None, every, defer="none")
    assert renb >= 1
    for step in every:
        assert np.array_equal(a[step][0], b[step][0]) and np.array_equal(a[step][2], b[step][2]), step
        assert a[step][1] == [1.0, 1.0]


@gpu
def test_deferred_and_undeferred_runs_agree_bit_for_bit_and_two_runs_are_identical():
    """REBO-MoS, whose forces are added in a fixed order (the alloy's three-body forces use float atomics: its runs agree
    to rounding with or without sources, tests/test_gpu_langevin_baths.py).  With sources on both orders launch the same
    kernels: final half, sums, control, apply, initial half"""
    s, v0, by_tag, g, groups, x_in, flux = _case("rebomos")
    mixed, _ = _two_sources_run("rebomos", EVERY_ODD)
    runs = [_resident("rebomos", _dev_sources("rebomos"), EVERY_ODD, defer=d)[0] for d in ("all", "none", "none")]
    for step in EVERY_ODD:
        for r in runs:
            assert np.array_equal(mixed[step][0], r[step][0]) and np.array_equal(mixed[step][2], r[step][2]), step
            assert mixed[step][1] == r[step][1], step


# ---- 3. host-linked mode ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("style", ["aeam", "rebomos"])
def test_hostlinked_sources_from_shuffled_atoms(oracle, style, capsys):
    """mdp_hnve_* with mdp_hnve_set_mask: the host's atom order is a shuffle of the tags, host reneighborings every 50
    steps re-upload atoms, velocities and mask (each upload counts the sources' atoms again).  Same reference, same bounds"""
    import ctypes as C
    s, v0, by_tag, g, groups, x_in, flux = _case(style)
    host = _reference(oracle, style)
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
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: no mask covers the current atoms"):
            c.heat_setup(_dev_sources(style), mvv2e=S.MVV2E)
        c.hnve_set_mask(mask_p)
        c.heat_setup(_dev_sources(style), mvv2e=S.MVV2E)
        c.heat_run(0)
        compute()
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
                sc = [c.heat_state(k)["scale"] for k in range(2)]
                got = c.hnve_download(s.n, want=("x", "v"))
                xd, vd = np.zeros((s.n, 3)), np.zeros((s.n, 3))
                xd[tag_p - 1], vd[tag_p - 1] = got["x"], got["v"]
                dev[step] = (xd, sc, vd)
        st = c.heat_state(0)
        assert st["applied"] == NSTEPS and st["error_step"] == -1
        assert st["mass"] == pytest.approx(float(s.mass[s.type][groups[0]].sum()), rel=1e-13)
    finally:
        c.close()
    assert uploads >= 3
    with capsys.disabled():
        _compare(s, host, dev, g, x_in, v0, f"source and sink, host-linked {style}, shuffled host order ({uploads} uploads)", EVERY20)


# ---- 4. one application in isolation; a sink that runs dry --------------------------------------------------------------
def _one_step(sources, after=None):
    """one step from the state of the case on a fresh brick, final half on its own: (x, v by tag, [state of source k])"""
    s, v0, by_tag, g, groups, x_in, flux = _case("rebomos")
    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        if sources is not None:
            d.heat(sources, first=0)
        d.compute(1, 0)
        d.step(0, 0, rebuild=False, defer_final=False)
        if after is not None:
            return after(ctx, d)
        states = [d.heat_state(k) for k in range(len(sources))] if sources is not None else []
        x, v = _by_tag(ctx, d, s)
        return x, v, states
    finally:
        ctx.close()


_OFF = []


def _without_sources():
    if not _OFF:
        _OFF.append(_one_step(None))
    return _OFF[0]


@gpu
def test_one_application_is_scale_v_minus_vsub_on_the_group_and_nothing_elsewhere():
    s, v0, by_tag, g, groups, x_in, flux = _case("rebomos")
    x_on, v_on, states = _one_step(_dev_sources("rebomos"))
    x_off, v_off, _ = _without_sources()
    assert np.array_equal(x_on, x_off)
    other = ~(groups[0] | groups[1])
    assert np.array_equal(v_on[other], v_off[other])
    m = s.mass[s.type]
    for k, l in enumerate(groups):
        st = states[k]
        assert st["applied"] == 1 and st["error_step"] == -1
        assert (st["scale"] > 1.0) == (k == 0) and st["scale"] != 1.0
        vsub = (st["scale"] - 1.0) * st["vcm"]
        want = st["scale"] * v_off[l] - vsub
        err = np.abs(v_on[l] - want) / (np.abs(st["scale"] * v_off[l]) + np.abs(vsub))
        assert err.max() <= 1e-15, (k, err.max())
        # the device's own sums are those of the state the step left
        vcm = (m[l][:, None] * v_off[l]).sum(axis=0) / m[l].sum()
        assert np.allclose(st["vcm"], vcm, rtol=0.0, atol=1e-12 * np.abs(v_off[l]).max())
        assert st["kecm"] == pytest.approx(heatref.kecm(v_off, m, l, S.FTM2V, S.MVV2E), rel=1e-12)
        assert st["mass"] == pytest.approx(float(m[l].sum()), rel=1e-13)
        # ... and the group gained eflux dt about its centre of mass
        assert _kecm(s, v_on, l) - _kecm(s, v_off, l) == pytest.approx(flux[k] * DT, rel=1e-9)
    assert np.all((states[1]["scale"] - 1.0) * states[1]["vcm"] != 0.0)     # (the sink drifts: vsub is exercised)


@gpu
def test_a_sink_that_runs_dry_is_a_handled_error_and_heat_off_gives_the_context_back():
    s, v0, by_tag, g, groups, x_in, flux = _case("rebomos")
    dry = [dict(eflux=flux[0], nevery=1, bit=SRC_BIT), dict(eflux=-2.0 * _kecm(s, v0, groups[1]) / DT, nevery=1, bit=SINK_BIT)]

    def after(ctx, d):
        for call in (d.thermo, lambda: ctx.md_download(d.nlocal, want=("v",)), lambda: d.heat_state(0), ctx.sync):
            with pytest.raises(capi.MdpError, match=r"fix heat kinetic energy went negative \(source 1, step 1\)") as e:
                call()
            assert e.value.code == -6                       # MDP_ESTATE
        d.heat_off()
        x, v = _by_tag(ctx, d, s)
        d.step(1, 0, rebuild=False, defer_final=False)      # a plain step runs
        t = d.thermo()
        assert np.isfinite(t["ke"]) and t["ke"] > 0.0
        with pytest.raises(capi.MdpError, match="mdp_heat_setup not called"):
            ctx.heat_state(0)
        return x, v
    x, v = _one_step(dry, after)
    x_off, v_off, _ = _without_sources()
    assert np.array_equal(x, x_off) and np.array_equal(v, v_off)   # neither source was applied: v is what the step left


# ---- 6. four slots, four nevery, first != 0; two runs on one context; the control workgroup's second trip ----------------
BITS4 = (16, 4, 32, 8)          # slot k's group: bathsref.masks4's A, B, C, D on these bits -- slot k does not hold the k-th lowest
C4 = (1e-3, -1e-3, 2e-3, -5e-4)
_CASE4 = []


def _case4():
    """the REBO-MoS case with four sources: (system, v0 with a drift on B and D, mask by tag, integrate group, [A, B, C, D],
    wrapped positions, [eflux])"""
    if not _CASE4:
        s, v0 = _system("rebomos")
        _, g, groups = bathsref.masks4(s)
        bathsref.check_masks(s, g, groups)
        by_tag = np.zeros(int(s.tag.max()) + 1, dtype=np.int32)
        m = bathsref.ALL_BIT | np.where(g, GBIT, 0)
        for bit, l in zip(BITS4, groups):
            m = m | np.where(l, bit, 0)
        by_tag[s.tag] = m
        v0 = v0.copy()
        v0[groups[1]] += DRIFT
        v0[groups[3]] -= 2.0 * DRIFT
        flux = [c * _kecm(s, v0, l) / DT for c, l in zip(C4, groups)]
        _CASE4.append((s, v0, by_tag, g, groups, S.wrap(s.box, s.x), flux))
    return _CASE4[0]


def _xsv(run):
    return {n: q[:3] for n, q in run.items()}


def _states(read, n):
    return [read(k) for k in range(n)]


def _compare_states(what, host, dev, every):
    """scale (STOL), vcm and ke of every source's LAST application and its application count, at every read.  vcm and ke
    are held to the `heat` net's limits for the same words (nets.HEAT_VCM_LIMIT, absolute in A/ps, and nets.HEAT_KE_LIMIT,
    relative: 100 times what the order of a source's sum does to them in the reference)"""
    ws = wc = wk = 0.0
    for step in every:
        for k, (a, b) in enumerate(zip(dev[step][3], host[step][3])):
            assert a["applied"] == b["applied"], (what, step, k, a["applied"], b["applied"])
            assert a["error_step"] == -1
            ws = worse(ws, abs(a["scale"] - b["scale"]) / abs(b["scale"]))
            wc = worse(wc, float(np.abs(a["vcm"] - b["vcm"]).max()))
            wk = worse(wk, abs(a["kecm"] - b["kecm"]) / abs(b["kecm"]) if b["kecm"] else abs(a["kecm"]))
            if b["applied"] == 0:
                assert a["scale"] == 1.0 and not a["vcm"].any() and a["kecm"] == 0.0, (what, step, k)
    print(f"{what}: state words, worst scale {ws:.2e} relative, vcm {wc:.2e} A/ps, ke {wk:.2e} relative")
    assert ws < STOL and wc < nets.HEAT_VCM_LIMIT and wk < nets.HEAT_KE_LIMIT, (ws, wc, wk)


def _resident4(sources, nsteps, every, first, cut=None):
    """one resident brick of the four-source case.  A read at an even step finds its final half deferred (the state read
    completes it); cut = (k, completed): mdp_heat_run(first + k) behind step k, whose final half is left pending across the
    call unless `completed`.  {step: (x, [scale], v, [state])} by tag"""
    s, v0, by_tag, g, groups, x_in, flux = _case4()
    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        d.heat(sources, first=first)
        d.compute(1, 0)
        out = {}
        for step in range(1, nsteps + 1):
            ev = step in every
            defer = step % 2 == 0 if ev else True
            if cut is not None and step == cut[0]:
                assert not ev
                defer = not cut[1]
            d.step(0, 0, rebuild="auto", defer_final=defer)
            if ev:
                sts = _states(d.heat_state, len(sources))
                x, v = _by_tag(ctx, d, s)
                out[step] = (x, [q["scale"] for q in sts], v, sts)
            if cut is not None and step == cut[0]:
                d.heat_run(first + step)       # a pending final half completes inside, without the sources
        return out
    finally:
        ctx.close()


@gpu
def test_four_sources_with_four_nevery_from_first_seven(oracle, capsys):
    """slots 2 and 3 of heat_src, of the apply kernel's select and of the sums; a `due` word that is partial at most steps
    (nevery 1, 2, 3, 5: full only where 30 divides the step); first = 7, so step n of the run is due where (7 + n) % nevery
    == 0.  60 steps, the state read at EVERY step: a source that was not due reports its previous application, and the
    application counts are exact"""
    s, v0, by_tag, g, groups, x_in, flux = _case4()
    nevery, first, nsteps = (1, 2, 3, 5), 7, 60
    every = tuple(range(1, nsteps + 1))
    make, rebuild_every = _oracle_engine(oracle, "rebomos")
    host, lowest = heatref.host_heat(make, s, v0, nsteps, set(every), rebuild_every, g,
                                     [dict(group=l, eflux=f, nevery=ne) for l, f, ne in zip(groups, flux, nevery)], dt=DT, first=first,
                                     skin=2.0, states=True)
    assert lowest > 0.5
    dev = _resident4([dict(eflux=f, nevery=ne, bit=b) for f, ne, b in zip(flux, nevery, BITS4)], nsteps, every, first)
    with capsys.disabled():
        _compare(s, _xsv(host), _xsv(dev), g, x_in, v0, "four sources, nevery 1 2 3 5, first 7", every)
        _compare_states("four sources, nevery 1 2 3 5, first 7", host, dev, every)
    assert [q["applied"] for q in dev[nsteps][3]] == [60, 30, 20, 12]
    # at step 1 (8 = 7 + 1) sources 0 and 1 alone were due; a source that is not due keeps what it reported
    assert [q["applied"] for q in dev[1][3]] == [1, 1, 0, 0]
    a, b = dev[4][3][2], dev[2][3][2]      # source 2 (nevery 3) is due at steps 2, 5, ...: at 3 and 4 it reports step 2's words
    assert (a["scale"], a["kecm"], a["applied"]) == (b["scale"], b["kecm"], 1) and np.array_equal(a["vcm"], b["vcm"])
    assert dev[5][3][2]["applied"] == 2 and dev[5][3][2]["kecm"] != b["kecm"]
    assert all(q["scale"] != 1.0 for q in dev[nsteps][3])


_REF2 = {}


@gpu
@pytest.mark.parametrize("path", ["resident-pending", "resident-completed", "hostlinked"])
def test_two_runs_in_a_row_on_one_context(oracle, path, capsys):
    """mdp_heat_run a second time, at step 30 of 60, which is due for all four sources (nevery 3, 5, 2, 1): step 30 belongs
    to the first run and is heated once -- not again as the second run's first step, whose counter starts at 30.  Resident
    with the seam's final half left pending across the call it completes there WITHOUT the sources (what INTEGRATION.md
    says of a final half pending at mdp_heat_run): the reference skips the applications of step 30 then.  Host-linked
    (mdp_hnve_final has run) and resident with the half completed: heated"""
    s, v0, by_tag, g, groups, x_in, flux = _case4()
    nevery, nsteps, k = (3, 5, 2, 1), 60, 30
    every = (7, 29, 31, 33, 45, 60)
    completed = path != "resident-pending"
    if completed not in _REF2:
        make, rebuild_every = _oracle_engine(oracle, "rebomos")
        _REF2[completed] = heatref.host_heat(make, s, v0, nsteps, set(every), rebuild_every, g,
                                             [dict(group=l, eflux=f, nevery=ne) for l, f, ne in zip(groups, flux, nevery)], dt=DT,
                                             cut=(k, completed), skin=2.0, states=True)
    host, lowest = _REF2[completed]
    assert lowest > 0.5
    sources = [dict(eflux=f, nevery=ne, bit=b) for f, ne, b in zip(flux, nevery, BITS4)]
    if path != "hostlinked":
        dev = _resident4(sources, nsteps, every, 0, cut=(k, completed))
    else:
        dev = _hostlinked4(oracle, sources, nsteps, every, k)
    with capsys.disabled():
        _compare(s, _xsv(host), _xsv(dev), g, x_in, v0, f"two runs, {path}", every)
        _compare_states(f"two runs, {path}", host, dev, every)
    assert [q["applied"] for q in dev[nsteps][3]] == ([20, 12, 30, 60] if completed else [19, 11, 29, 59])


def _hostlinked4(oracle, sources, nsteps, every, k):
    """the four-source case host-linked from shuffled atoms, mdp_heat_run(k) behind step k"""
    s, v0, by_tag, g, groups, x_in, flux = _case4()
    perm = np.random.default_rng(17).permutation(s.n)
    type_p, tag_p = s.type[perm].copy(), s.tag[perm].copy()
    mask_p, gp, skin = by_tag[tag_p], g[perm], 2.0
    c = capi.Context(0)
    try:
        P = oracle.rebomos_params(POT_REBOMOS)
        c.rebomos_set_params(ob.product_rebomos_params(P))
        cut = P.cut3rebo + skin

        def upload(x, v):
            xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), type_p, tag_p, s.mass), cut)
            c.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=[0, 0, 1])
            c.set_skin(skin)
            c.hnve_upload_v(v)
            c.hnve_set_mask(mask_p)
        c.set_box_host(s.box)
        c.hnve_setup(DT, S.FTM2V, s.mass)
        c.integrate_group(GBIT)
        upload(x_in[perm].copy(), v0[perm])
        c.heat_setup(sources, mvv2e=S.MVV2E)
        c.heat_run(0)
        c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
        dev = {}
        for step in range(1, nsteps + 1):
            moved, late = c.hnve_initial()
            if moved or step % 25 == 0:
                got = c.hnve_download(s.n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]
                upload(xw, got["v"])
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
            c.hnve_final()
            if step in every:
                sts = _states(c.heat_state, len(sources))
                got = c.hnve_download(s.n, want=("x", "v"))
                xd, vd = np.zeros((s.n, 3)), np.zeros((s.n, 3))
                xd[tag_p - 1], vd[tag_p - 1] = got["x"], got["v"]
                dev[step] = (xd, [q["scale"] for q in sts], vd, sts)
            if step == k:
                c.heat_run(k)
        return dev
    finally:
        c.close()


def _fma(a, b, c):
    """fl(a b + c) with ONE rounding, elementwise: Dekker's exact product and Knuth's exact sum give a b + c = s + t + e
    exactly; s + (t + e) is then the rounded value except in rare ties, which the caller settles with _fma_exact"""
    split = 134217729.0 * a
    ah = split - (split - a)
    al = a - ah
    split = 134217729.0 * b
    bh = split - (split - b)
    bl = b - bh
    p = a * b
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def _fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _big_step(sources, s, v0, by_tag):
    """one step of the 275 684-atom alloy on a fresh brick, final half on its own: (v by tag, [state of source k])"""
    ctx, st, cutghost, skin, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(by_tag, GBIT)
        if sources is not None:
            d.heat(sources, first=0)
        d.compute(0, 0)
        d.step(0, 0, rebuild=False, defer_final=False)
        states = [d.heat_state(k) for k in range(len(sources))] if sources is not None else []
        got = ctx.md_download(d.nlocal, want=("v",))
        v = np.zeros((s.n, 3))
        v[d.tags_local - 1] = got["v"]
        return v, states
    finally:
        ctx.close()


@gpu
def test_the_control_workgroups_second_trip_against_fsum(capsys):
    """275 684 aluminium atoms (fcc 41^3): heat_sums_kernel leaves 270 partial slots, so mdp_slot_sum_256<kHeatW> of the control
    workgroup takes a second trip (the Langevin sums have the 70 304-atom case for theirs), and the last block holds 228
    atoms: its first j only.  Four sources on tag classes modulo 8 inside an integrate group that leaves tag % 7 == 0 held,
    each with a drift of its own.  One step; the velocities before the application come from a twin without sources.
    scale, vcm and ke of every source against math.fsum over them to STOL = 1e-12 relative (any order of adding 275 684
    terms stays within n 2^-53 = 3.1e-11; the device's fixed tree and fsum over ~30 000 terms of one sign for ke and m, and
    a vcm that the drift keeps at some tenths of A/ps, do far better: measured below).  Every source atom's new velocity is
    fma(scale, v, -vsub) of the downloaded words bit for bit; every other atom's is the twin's bit for bit."""
    af = capi.AeamFile(POT_AEAM)
    s = S.fcc_cell(4.045, 41)      # (aluminium alone: no three-body forces, whose float atomics would make the twin differ)
    s.mass[1:3] = af.mass[:2]
    assert s.n == 275684 and -(-s.n // 1024) == 270 and s.n % 1024 == 228
    v0 = S.gaussian_velocities(s, 300.0, seed=95)
    g = s.tag % 7 != 0
    groups = [g & (s.tag % 8 == r) for r in (1, 2, 5, 6)]
    drifts = [np.array(q) for q in ((0.5, -0.3, 0.2), (-0.4, 0.6, 0.3), (0.2, 0.3, -0.7), (-0.6, -0.2, -0.4))]
    for l, dr in zip(groups, drifts):
        v0[l] += dr
    by_tag = np.zeros(s.n + 1, dtype=np.int32)
    m = bathsref.ALL_BIT | np.where(g, GBIT, 0)
    for bit, l in zip(BITS4, groups):
        m = m | np.where(l, bit, 0)
    by_tag[s.tag] = m
    mass = s.mass[s.type]
    flux = [c * heatref.kecm(v0, mass, l, S.FTM2V, S.MVV2E) * S.MVV2E / DT for c, l in zip(C4, groups)]
    v_on, states = _big_step([dict(eflux=f, nevery=1, bit=b) for f, b in zip(flux, BITS4)], s, v0, by_tag)
    v_off, _ = _big_step(None, s, v0, by_tag)
    other = ~np.logical_or.reduce(groups)
    assert np.array_equal(v_on[other], v_off[other]), "an atom of no source changed"
    assert np.array_equal(v_off[~g], v0[~g])
    worst = dict(scale=0.0, vcm=0.0, ke=0.0, mass=0.0)
    for k, l in enumerate(groups):
        st = states[k]
        assert st["applied"] == 1 and st["error_step"] == -1
        ml, vl = mass[l], v_off[l]
        M = math.fsum(ml)
        vcm = np.array([math.fsum(ml * vl[:, c]) for c in range(3)]) / M
        ke = (0.5 * S.MVV2E * math.fsum(ml * (vl * vl).sum(axis=1))) * S.FTM2V
        den = ke - 0.5 * float(vcm @ vcm) * M
        assert den > 0.9 * ke                              # (ke - t keeps its digits: the drift is small against the thermal motion)
        scale = math.sqrt((den + flux[k] * DT * S.FTM2V) / den)
        worst["scale"] = max(worst["scale"], abs(st["scale"] - scale) / scale)
        worst["vcm"] = max(worst["vcm"], float((np.abs(st["vcm"] - vcm) / np.abs(vcm)).max()))
        worst["ke"] = max(worst["ke"], abs(st["kecm"] - den) / den)
        worst["mass"] = max(worst["mass"], abs(st["mass"] - M) / M)
        assert (st["scale"] > 1.0) == (C4[k] > 0.0) and st["scale"] != 1.0
        # the rescaled velocities, from the words the control workgroup left
        sc = np.float64(st["scale"])
        vsub = (sc - 1.0) * st["vcm"]
        assert np.all(vsub != 0.0)
        want = _fma(sc, vl, -vsub[None, :])
        for i, c in zip(*np.nonzero(v_on[l] != want)):     # (ties of the vectorised form: settled exactly)
            want[i, c] = _fma_exact(float(sc), float(vl[i, c]), -float(vsub[c]))
        assert np.array_equal(v_on[l], want), (k, int((v_on[l] != want).sum()))
    with capsys.disabled():
        print("275 684 atoms, four sources against fsum: " + ", ".join(f"{q} {w:.2e}" for q, w in worst.items()) + " relative")
    assert all(w < STOL for w in worst.values()), worst


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
@gpu
def test_library_refusals():
    s, v0, by_tag, g, groups, x_in, flux = _case("rebomos")
    ok = _dev_sources("rebomos")
    src = lambda k=0, **kw: dict(ok[k], **kw)       # noqa: E731
    c = capi.Context(0)
    try:
        with pytest.raises(capi.MdpError, match="0 sources; a context takes 1 to 4") as e:
            c.heat_setup([])
        assert e.value.code == -1                           # MDP_EINVAL
        with pytest.raises(capi.MdpError, match="5 sources; a context takes 1 to 4"):
            c.heat_setup([src(0, bit=4 << k) for k in range(5)])
        with pytest.raises(capi.MdpError, match="source 1 has group bit 0"):
            c.heat_setup([src(0), src(1, bit=0)])
        with pytest.raises(capi.MdpError, match="sources 0 and 1 share the group bit 4"):
            c.heat_setup([src(0), src(1, bit=4 | 8)])
        with pytest.raises(capi.MdpError, match="source 1: nevery must be >= 1"):
            c.heat_setup([src(0), src(1, nevery=0)])
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(capi.MdpError, match="source 0: eflux must be finite"):
                c.heat_setup([src(0, eflux=bad)])
        with pytest.raises(capi.MdpError, match="mdp_heat_setup not called") as e:
            c.heat_run(0)
        assert e.value.code == -6                           # MDP_ESTATE
        with pytest.raises(capi.MdpError, match="mdp_heat_setup not called"):
            c.heat_state(0)
        c.heat_off()                                        # (nothing is on: nothing to do)
    finally:
        c.close()

    ctx, st, cutghost, skin, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0.copy())
        d.compute(1, 0)
        # no mask; an empty source; atoms in two sources; source atoms outside the integrate group (counted on the device)
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: no mask covers the current atoms") as e:
            d.heat(ok)
        assert e.value.code == -6
        d.set_group(by_tag, GBIT)
        with pytest.raises(capi.MdpError, match=r"heat source 1 has no atoms \(group bit 64\)"):
            d.heat([src(0), src(1, bit=64)])
        over = by_tag.copy()
        both = groups[0] & (s.tag % 8 == 0)
        over[s.tag[both]] |= SINK_BIT
        n_over = int(both.sum())
        assert n_over > 5
        d.set_group(over, GBIT)
        with pytest.raises(capi.MdpError, match=f"mdp_heat_setup: {n_over} atoms are in more than one of the 2 heat sources"):
            d.heat(ok)
        out = by_tag.copy()
        held = ~g & (s.tag % 7 == 0)
        out[s.tag[held]] |= SRC_BIT
        n_out = int(held.sum())
        assert n_out > 5
        d.set_group(out, GBIT)
        with pytest.raises(capi.MdpError, match=f"mdp_heat_setup: {n_out} atoms of the heat sources .* are outside the integrate group"):
            d.heat(ok)
        # ... and by a mask upload while the sources are on
        d.set_group(by_tag, GBIT)
        d.heat(ok)
        with pytest.raises(capi.MdpError, match=f"mdp_md_set_mask: {n_over} atoms are in more than one of the 2 heat sources"):
            d.set_group(over, GBIT)
        with pytest.raises(capi.MdpError, match=f"mdp_md_set_mask: {n_out} atoms of the heat sources"):
            d.set_group(out, GBIT)
        d.set_group(by_tag, GBIT)
        with pytest.raises(capi.MdpError, match="source index 2 out of range"):
            ctx.heat_state(2)
        # a thermostat or the minimiser, in either order
        with pytest.raises(capi.MdpError, match="mdp_nhc_setup: heat sources"):
            ctx.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_langevin_setup: heat sources"):
            d.langevin(300.0, 300.0, 0.1, 4711)
        with pytest.raises(capi.MdpError, match="mdp_langevin_baths: heat sources"):
            ctx.langevin_baths([dict(t_start=300.0, t_stop=300.0, t_period=0.1, seed=7, natoms=10, bit=4),
                                dict(t_start=300.0, t_stop=300.0, t_period=0.1, seed=8, natoms=10, bit=8)])
        with pytest.raises(capi.MdpError, match="mdp_fire_setup: heat sources"):
            ctx.fire_setup(0.0, 0.0, BIG, BIG)
        d.heat_off()
        ctx.nhc_setup(300.0, 300.0, 0.1, 30.0)
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: the Nose-Hoover chain"):
            d.heat(ok)
        ctx.nhc_off()
        d.langevin(300.0, 300.0, 0.1, 4711)
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: the Langevin thermostat"):
            d.heat(ok)
        d.langevin_off()
        ctx.fire_setup(0.0, 0.0, BIG, BIG)
        with pytest.raises(capi.MdpError, match="mdp_heat_setup: a minimisation"):
            d.heat(ok)
        ctx.fire_off()
        d.heat(ok)                                          # (with all of them off the sources go on)
        d.heat_off()
    finally:
        ctx.close()

    # a brick of several ranks, in either call order
    p = capi.read_rebomos_file(POT_REBOMOS)
    cutghost = 3.0 * p.rcmax[0][0] + 2.0
    for sources_first in (True, False):
        c = capi.Context(0)
        try:
            c.rebomos_set_params(p)
            d = resident.DeviceDomain(c, capi.STYLE_REBOMOS, s, cutghost, 2.0, [0, 0, 1], v0=v0.copy())
            d.set_group(by_tag, GBIT)
            if sources_first:
                c.heat_setup(ok, mvv2e=S.MVV2E)
                with pytest.raises(capi.MdpError, match=r"mdp_dd_setup: heat sources \(mdp_heat_setup\) run on one rank only"):
                    c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
            else:
                c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
                with pytest.raises(capi.MdpError, match="mdp_heat_setup: heat sources run on one rank only"):
                    c.heat_setup(ok, mvv2e=S.MVV2E)
        finally:
            c.close()
