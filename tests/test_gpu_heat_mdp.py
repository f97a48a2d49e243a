"""GPU: constant-flux heat sources on groups (mdp_heat_setup / _run / _state / _off; heat_sums_kernel, heat_control_kernel
and heat_apply_kernel of csrc/heat.hip behind every final half) against the masked host loop of tests/heatref.py around the
ORACLE forces.

The two cells of the several-bath tests at 300 K, 200 steps of 0.001 ps with rebuild="auto" and a 0.5 A skin.  The masks are
bathsref.masks: bath A (bit 4) is the source, bath B (bit 8) the sink, bath C's atoms are plain integrated atoms, a third of
the cell is held.  B's atoms carry an extra drift of (0.5, -0.3, 0.2) A/ps, so that vsub = (scale - 1) vcm is exercised.
eflux_k = +-1e-3 KEcm_k(0) / dt.  Tolerances are the project's own for these cells and step counts under a global-sum
feedback: positions 1e-9 A (the grouped thermostats), velocities 2e-8 A/ps (VTOL of tests/test_gpu_langevin_mdp.py, the
one velocity bound those tests hold against a host loop), held atoms bit for bit, the scale 1e-12 relative.  The reference
with every source's atoms summed in a permuted order stays 100 times inside them (test_a_permuted_sum_..., no GPU)."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from firerig import BIG
from refloops import worse
import bathsref
import heatref
import mdref
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
