"""GPU: the Langevin thermostat of the integrate calls (mdp_langevin_*, csrc/langevin.hip) against velocity Verlet plus
the NumPy thermostat (tests/langevinref.py: the same Philox noise keyed by tag and step) around the ORACLE forces, on
the resident path (mdp_md_integrate_check with the fused final half, device reneighborings, thermo reads at odd
intervals that complete deferred final halves or leave a final half to run on its own) and on the host-linked path
(mdp_hnve_*, host reneighborings); bitwise determinism; the same trajectory by tag from shuffled atoms;
mdp_langevin_off giving back NVE; the library's refusals."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
import langevinref
import mdref
import oracle_bindings as ob

pytestmark = pytest.mark.gpu

DAMP = 0.05    # ps: a short coupling time, so that 200 steps of the thermostat move the trajectory
SEED = 48271
CASES = {  # Tstart, Tstop, scale ratios, zero, tally
    "tally": (300.0, 300.0, None, False, True),
    "ramp-scale-zero-tally": (300.0, 900.0, {1: 2.0, 2: 0.5}, True, True),
}


def _lgv(s, case, dt=0.001):
    t0, t1, ratio, zero, tally = case
    return langevinref.Langevin(t0, t1, DAMP, SEED, s.mass, dt, S.FTM2V, boltz=S.BOLTZ, mvv2e=S.MVV2E, ratio=ratio,
                                zero=zero, tally=tally)


def _host_lgv(make_engine, s, v0, nsteps, every, rebuild_every, lgv, dt=0.001):
    """velocity Verlet + Langevin around the oracle; {step: (x by tag, thermostat energy)}"""
    m = s.mass[s.type][:, None]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    lgv.setup(0, nsteps)
    f = eng.compute(x, eflag=1, vflag=0)["f_owned"] + lgv.force(0, s.tag, s.type, v, phase=1)
    lgv.tally_setup(v)
    dtf = 0.5 * dt * S.FTM2V
    out = {}
    for step in range(1, nsteps + 1):
        v += dtf * f / m
        x += dt * v
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"] + lgv.force(step, s.tag, s.type, v)
        v += dtf * f / m
        lgv.tally_step(v)
        if step in every:
            out[step] = (x.copy(), lgv.scalar(), v.copy())
    return out


def _compare(s, host, dev, xtol=1e-9, etol=1e-9):
    worst_x = worst_e = 0.0
    for step in sorted(host):
        xh, eh = host[step][:2]
        xd, ed = dev[step][:2]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        worst_x = max(worst_x, float(np.abs(dx).max()))
        worst_e = max(worst_e, abs(ed - eh))
    assert worst_x < xtol, worst_x
    assert worst_e < etol, worst_e
    return worst_x, worst_e


def _rebomos():
    s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
    return s, S.gaussian_velocities(s, 300.0, seed=91)


def _aeam():
    af = capi.AeamFile(POT_AEAM)
    s = S.fcc_cell(4.045, 6, frac_type2=0.0075, seed=92)
    s.mass[1:3] = af.mass[:2]
    return s, S.gaussian_velocities(s, 300.0, seed=93)


def _domain(style, s, v0):
    ctx = capi.Context(0)
    if style == capi.STYLE_REBOMOS:
        p = capi.read_rebomos_file(POT_REBOMOS)
        ctx.rebomos_set_params(p)
        skin, cutghost, map_ = 2.0, 3.0 * p.rcmax[0][0] + 2.0, [0, 0, 1]
    else:
        af = capi.AeamFile(POT_AEAM)
        tabs = af.build()
        ctx.aeam_set_tables(tabs)
        skin, cutghost, map_ = 1.0, float(af.cut_table(tabs).max()) + 1.0, None
    return ctx, resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)


# thermo reads at odd steps: a multiple of 14 leaves the final half to the next read (deferred, completed by the
# tally read), the others run it on their own (f + f_L written back for the next initial half)
EVERY = (7, 14, 21, 49, 98, 133, 140, 161, 200)


def _resident(style, s, v0, case, nsteps=200, every=EVERY):
    t0, t1, ratio, zero, tally = case
    ctx, d = _domain(style, s, v0)
    d.langevin(t0, t1, DAMP, SEED, ratio=ratio, zero=zero, tally=tally, first=0, last=nsteps)
    d.compute(1, 0)
    out = {}
    for step in range(1, nsteps + 1):
        ev = step in every
        d.step(1 if ev else 0, 0, rebuild="auto", defer_final=(not ev) or step % 14 == 0)
        if ev:
            e = d.langevin_tally()
            got = ctx.md_download(d.nlocal, want=("x", "v"))
            x = np.zeros((s.n, 3))
            x[d.tags_local - 1] = got["x"]
            vv = np.zeros((s.n, 3))
            vv[d.tags_local - 1] = got["v"]
            out[step] = (x, e, vv)
    return out, d, ctx


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_resident_langevin_follows_the_host_reference(oracle, style, case):
    if style == "rebomos":
        s, v0 = _rebomos()
        P = oracle.rebomos_params(POT_REBOMOS)
        make, rebuild_every, st = (lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)), 50, capi.STYLE_REBOMOS
    else:
        s, v0 = _aeam()
        T = oracle.aeam_pot(POT_AEAM)
        make, rebuild_every, st = (lambda sy: mdref.AeamCPU(oracle, T, sy, skin=1.0)), 25, capi.STYLE_AEAM
    host = _host_lgv(make, s, v0, 200, EVERY, rebuild_every, _lgv(s, CASES[case]))
    dev, d, ctx = _resident(st, s, v0, CASES[case])
    ctx.close()
    if style == "aeam":
        assert d.builds > 1                     # the device reneighbored on its own (skin 1.0 A at 300 K)
    _compare(s, host, {k: w[:2] for k, w in dev.items()})
    assert abs(host[200][1]) > 1e-3             # the thermostat exchanged energy


def test_hostlinked_langevin_follows_the_host_reference(oracle):
    """mdp_hnve_* with the thermostat: host reneighborings every 50 steps (download, new atoms, mdp_hnve_upload_v)"""
    P = oracle.rebomos_params(POT_REBOMOS)
    s, v0 = _rebomos()
    nsteps, every, rebuild_every = 200, (20, 40, 60, 80, 100, 120, 140, 160, 180, 200), 50
    for case in CASES.values():
        t0, t1, ratio, zero, tally = case
        host = _host_lgv(lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0), s, v0, nsteps, every, rebuild_every,
                         _lgv(s, case))
        c = capi.Context(0)
        c.rebomos_set_params(ob.product_rebomos_params(P))
        c.set_box_host(s.box)
        x = S.wrap(s.box, s.x)
        eng = mdref.RebomosCPU(oracle, P, S.System(s.box, x.copy(), s.type, s.tag, s.mass), skin=2.0)
        c.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
        assert c.host_ghosts_derived()
        c.set_skin(2.0)
        c.hnve_setup(0.001, S.FTM2V, s.mass)
        c.langevin_setup(t0, t1, DAMP, SEED, s.n, ratio=ratio, zero=zero, tally=tally, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        c.langevin_run(0, nsteps)
        c.hnve_upload_v(v0)
        c.rebomos_compute_host(eng.nlocal, eflag=0, vflag=0)
        dev = {}
        for step in range(1, nsteps + 1):
            c.hnve_initial()
            if step % rebuild_every == 0:   # the host's reneighboring: atoms come up, are wrapped and go down again
                got = c.hnve_download(eng.nlocal, want=("x", "v"))
                x = S.wrap(s.box, got["x"])
                eng = mdref.RebomosCPU(oracle, P, S.System(s.box, x.copy(), s.type, s.tag, s.mass), skin=2.0)
                c.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
                c.hnve_upload_v(got["v"])
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
            c.hnve_final()
            if step in every:
                dev[step] = (c.hnve_download(eng.nlocal, want=("x",))["x"], c.langevin_tally())
        c.close()
        _compare(s, host, dev)


def test_resident_langevin_is_bitwise_reproducible():
    s, v0 = _rebomos()
    case = CASES["ramp-scale-zero-tally"]
    a, _, ca = _resident(capi.STYLE_REBOMOS, s, v0, case, nsteps=100)
    ca.close()
    b, _, cb = _resident(capi.STYLE_REBOMOS, s, v0, case, nsteps=100)
    cb.close()
    for step in a:
        assert np.array_equal(a[step][0], b[step][0])
        assert np.array_equal(a[step][2], b[step][2])
        assert a[step][1] == b[step][1]


def test_shuffled_atoms_give_the_same_trajectory_by_tag():
    """the noise is keyed by tag: atoms handed over in another order follow the same trajectories"""
    s, v0 = _aeam()
    case = CASES["tally"]
    a, _, ca = _resident(capi.STYLE_AEAM, s, v0, case)
    ca.close()
    perm = np.random.default_rng(5).permutation(s.n)
    s2 = S.System(s.box, s.x[perm].copy(), s.type[perm].copy(), s.tag[perm].copy(), s.mass)
    b, _, cb = _resident(capi.STYLE_AEAM, s2, v0[perm].copy(), case)
    cb.close()
    for step in a:
        dx = b[step][0] - a[step][0]
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        assert np.abs(dx).max() < 1e-12, (step, np.abs(dx).max())


def test_langevin_off_after_a_run_gives_back_nve(oracle):
    """Langevin for 60 steps, the last final half deferred; mdp_langevin_off completes it with its Langevin force (the
    velocities then are the reference's of step 60) and switches the thermostat off on the SAME context; after the
    forces of a new run (the last Langevin force stays in f, as in LAMMPS' atom->f) the next 100 steps follow velocity
    Verlet around the oracle (1e-9 A)"""
    P = oracle.rebomos_params(POT_REBOMOS)
    s, v0 = _rebomos()
    ref = _host_lgv(lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0), s, v0, 60, (60,), 50, _lgv(s, CASES["tally"]))
    _, d, ctx = _resident(capi.STYLE_REBOMOS, s, v0, CASES["tally"], nsteps=60, every=())
    assert d._final_pending
    d.langevin_off()
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    x = np.zeros((s.n, 3))
    v = np.zeros((s.n, 3))
    x[d.tags_local - 1] = got["x"]
    v[d.tags_local - 1] = got["v"]
    assert np.abs(v - ref[60][2]).max() < 1e-9      # the deferred final half ran with its Langevin force
    with pytest.raises(capi.MdpError, match="mdp_langevin_setup not called"):
        ctx.langevin_tally()                       # the thermostat is off
    d.compute(1, 0)                                # Verlet::setup of the next run
    for step in range(1, 101):
        d.step(0, 0, rebuild="auto", defer_final=step < 100)
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    xd = np.zeros((s.n, 3))
    xd[d.tags_local - 1] = got["x"]
    ctx.close()
    m = s.mass[s.type]
    xh, vh = S.wrap(s.box, x), v.copy()
    dtf = 0.5 * 0.001 * S.FTM2V
    eng = mdref.RebomosCPU(oracle, P, S.System(s.box, xh.copy(), s.type, s.tag, s.mass), skin=2.0)
    f = eng.compute(xh, eflag=1, vflag=0)["f_owned"]
    for step in range(1, 101):
        vh += dtf * f / m[:, None]
        xh += 0.001 * vh
        if step % 50 == 0:
            xh = S.wrap(s.box, xh)
            eng = mdref.RebomosCPU(oracle, P, S.System(s.box, xh.copy(), s.type, s.tag, s.mass), skin=2.0)
        f = eng.compute(xh, eflag=1, vflag=0)["f_owned"]
        vh += dtf * f / m[:, None]
    dx = xd - xh
    dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
    assert np.abs(dx).max() < 1e-9


def test_library_refusals():
    s, v0 = _rebomos()
    p = capi.read_rebomos_file(POT_REBOMOS)
    cutghost = 3.0 * p.rcmax[0][0] + 2.0
    # zero / tally on a brick of several ranks, in either order
    for kw in ({"zero": True}, {"tally": True}):
        for langevin_first in (True, False):
            c = capi.Context(0)
            c.rebomos_set_params(p)
            resident.DeviceDomain(c, capi.STYLE_REBOMOS, s, cutghost, 2.0, [0, 0, 1], v0=v0.copy())
            if langevin_first:
                c.langevin_setup(300.0, 300.0, 0.1, SEED, s.n, **kw)
                with pytest.raises(capi.MdpError, match="one rank only"):
                    c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
            else:
                c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
                with pytest.raises(capi.MdpError, match="one rank only"):
                    c.langevin_setup(300.0, 300.0, 0.1, SEED, s.n, **kw)
                c.langevin_setup(300.0, 300.0, 0.1, SEED, s.n)   # (without them a brick takes it)
            c.close()
    # one thermostat per context, in either order
    c = capi.Context(0)
    c.nhc_setup(300.0, 300.0, 0.1, 30.0)
    with pytest.raises(capi.MdpError, match="one thermostat per context"):
        c.langevin_setup(300.0, 300.0, 0.1, SEED, 11)
    c.nhc_off()
    c.langevin_setup(300.0, 300.0, 0.1, SEED, 11)
    with pytest.raises(capi.MdpError, match="one thermostat per context"):
        c.nhc_setup(300.0, 300.0, 0.1, 30.0)
    c.langevin_off()
    # bad numbers
    for args, kw in (((300.0, 300.0, 0.1, 0), {}), ((300.0, 300.0, 0.0, SEED), {}), ((300.0, 300.0, -0.1, SEED), {}),
                     ((-1.0, 300.0, 0.1, SEED), {}), ((300.0, -5.0, 0.1, SEED), {}),
                     ((300.0, 300.0, 0.1, SEED), {"ratio": {2: 0.0}}), ((300.0, 300.0, 0.1, SEED), {"ratio": {1: -1.0}})):
        with pytest.raises(capi.MdpError):
            c.langevin_setup(*args, 11, **kw)
    with pytest.raises(capi.MdpError, match="mdp_langevin_setup not called"):
        c.langevin_run(0, 10)
    c.close()
