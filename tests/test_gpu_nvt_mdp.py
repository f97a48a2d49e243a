"""GPU: the Nose-Hoover chain thermostat of the integrate calls (mdp_nhc_*, csrc/nhc.hip) against velocity Verlet plus the
NumPy chain (tests/nhcref.py) around the ORACLE forces, on the resident path (mdp_md_integrate_check with the fused
final half, device reneighborings) and on the host-linked path (mdp_hnve_*, host reneighborings); bitwise determinism
of the resident run; mdp_nhc_off after a run giving back NVE; the refusal of several ranks."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
import mdref
import nhcref
import oracle_bindings as ob

pytestmark = pytest.mark.gpu

CASES = [  # (tchain, tloop, drag, Tstart, Tstop)
    (3, 1, 0.0, 300.0, 300.0),
    (1, 1, 0.0, 300.0, 300.0),
    (4, 2, 0.2, 300.0, 300.0),
    (3, 1, 0.0, 300.0, 900.0),
]
TDAMP = 0.02   # ps: a short coupling time, so that 200 steps of the chain move the trajectory


def _host_nvt(make_engine, s, v0, nsteps, every, skin, rebuild_every, nhc, dt=0.001):
    """velocity Verlet + chain around the oracle; {step: (x by tag, thermostat energy, T)}"""
    m = s.mass[s.type]
    x = S.wrap(s.box, s.x)
    v = v0.copy()
    eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
    f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
    nhc.setup(v, m, 0, nsteps)
    dtf = 0.5 * dt * S.FTM2V
    out = {}
    for step in range(1, nsteps + 1):
        nhc.begin_step(step)
        v *= nhc.half()
        v += dtf * f / m[:, None]
        x += dt * v
        if step % rebuild_every == 0:
            x = S.wrap(s.box, x)
            eng = make_engine(S.System(s.box, x.copy(), s.type, s.tag, s.mass))
        f = eng.compute(x, eflag=1, vflag=0)["f_owned"]
        v += dtf * f / m[:, None]
        v *= nhc.half(nhc.temperature(v, m))
        if step % every == 0:
            out[step] = (x.copy(), nhc.energy(), nhc.T)
    return out


def _compare(s, host, dev, xtol=1e-9, etol=1e-9):
    worst_x = worst_e = 0.0
    for step in sorted(host):
        xh, eh, th = host[step]
        xd, ed, td = dev[step]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        worst_x = max(worst_x, float(np.abs(dx).max()))
        worst_e = max(worst_e, abs(ed - eh))
        assert td == pytest.approx(th, rel=1e-9)
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
    return s, S.gaussian_velocities(s, 300.0, seed=93), af


def _resident(style, s, v0, case, nsteps=200, every=20):
    tchain, tloop, drag, t0, t1 = case
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
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=v0)
    d.thermostat(t0, t1, TDAMP, tchain=tchain, tloop=tloop, drag=drag, first=0, last=nsteps)
    d.compute(1, 0)
    out = {}
    for step in range(1, nsteps + 1):
        ev = 1 if step % every == 0 else 0
        d.step(ev, 0, rebuild="auto", defer_final=not ev)
        if ev:
            st = d.thermostat_state()
            got = ctx.md_download(d.nlocal, want=("x", "v"))
            x = np.zeros((s.n, 3))
            x[d.tags_local - 1] = got["x"]
            vv = np.zeros((s.n, 3))
            vv[d.tags_local - 1] = got["v"]
            out[step] = (x, st["energy"], st["temp"], vv)
    return out, d, ctx


@pytest.mark.parametrize("case", CASES, ids=["chain3", "chain1", "chain4-loop2-drag", "ramp300-900"])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_resident_nvt_follows_the_host_chain(oracle, style, case):
    tchain, tloop, drag, t0, t1 = case
    if style == "rebomos":
        s, v0 = _rebomos()
        P = oracle.rebomos_params(POT_REBOMOS)
        make, skin, rebuild_every, st = (lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)), 2.0, 50, capi.STYLE_REBOMOS
    else:
        s, v0, _ = _aeam()
        T = oracle.aeam_pot(POT_AEAM)
        make, skin, rebuild_every, st = (lambda sy: mdref.AeamCPU(oracle, T, sy, skin=1.0)), 1.0, 25, capi.STYLE_AEAM
    nhc = nhcref.NHC(t0, t1, TDAMP, 3 * s.n - 3, 0.001, tchain=tchain, tloop=tloop, drag=drag, boltz=S.BOLTZ, mvv2e=S.MVV2E)
    host = _host_nvt(make, s, v0, 200, 20, skin, rebuild_every, nhc)
    dev, d, ctx = _resident(st, s, v0, case)
    ctx.close()
    _compare(s, host, {k: v[:3] for k, v in dev.items()})
    if t1 != t0:
        assert host[200][2] > 350.0     # the ramp pulls the temperature up


def test_hostlinked_nvt_follows_the_host_chain(oracle):
    """mdp_hnve_* with the thermostat: host reneighborings every 50 steps (download, new atoms, mdp_hnve_upload_v)"""
    P = oracle.rebomos_params(POT_REBOMOS)
    s, v0 = _rebomos()
    nsteps, every, rebuild_every = 200, 20, 50
    for case in CASES:
        tchain, tloop, drag, t0, t1 = case
        nhc = nhcref.NHC(t0, t1, TDAMP, 3 * s.n - 3, 0.001, tchain=tchain, tloop=tloop, drag=drag, boltz=S.BOLTZ,
                         mvv2e=S.MVV2E)
        host = _host_nvt(lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0), s, v0, nsteps, every, 2.0, rebuild_every,
                         nhc)
        c = capi.Context(0)
        c.rebomos_set_params(ob.product_rebomos_params(P))
        c.set_box_host(s.box)
        x = S.wrap(s.box, s.x)
        eng = mdref.RebomosCPU(oracle, P, S.System(s.box, x.copy(), s.type, s.tag, s.mass), skin=2.0)
        c.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
        assert c.host_ghosts_derived()
        c.set_skin(2.0)
        c.hnve_setup(0.001, S.FTM2V, s.mass)
        c.nhc_setup(t0, t1, TDAMP, 3 * s.n - 3, tchain=tchain, tloop=tloop, drag=drag, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        c.nhc_run(0, nsteps)
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
            if step % every == 0:
                st = c.nhc_state()
                dev[step] = (c.hnve_download(eng.nlocal, want=("x",))["x"], st["energy"], st["temp"])
        c.close()
        _compare(s, host, dev)


def test_resident_nvt_is_bitwise_reproducible():
    s, v0 = _rebomos()
    a, _, ca = _resident(capi.STYLE_REBOMOS, s, v0, CASES[0], nsteps=100)
    ca.close()
    b, _, cb = _resident(capi.STYLE_REBOMOS, s, v0, CASES[0], nsteps=100)
    cb.close()
    for step in a:
        assert np.array_equal(a[step][0], b[step][0])
        assert np.array_equal(a[step][3], b[step][3])
        assert a[step][1] == b[step][1] and a[step][2] == b[step][2]


def test_nhc_off_after_a_run_gives_back_nve(oracle):
    """NVT for 60 steps, the last final half deferred; mdp_nhc_off completes it and switches the chain off on the SAME
    context; its next 100 steps follow velocity Verlet around the oracle from the state it had then (1e-9 A), while the
    thermostat (Tdamp 0.02 ps) would have moved them far"""
    P = oracle.rebomos_params(POT_REBOMOS)
    s, v0 = _rebomos()
    _, d, ctx = _resident(capi.STYLE_REBOMOS, s, v0, CASES[0], nsteps=60, every=1000)
    assert d._final_pending                         # the last step left its final half to the next one
    d.thermostat_off()                              # ... which mdp_nhc_off ran, with the chain
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    x = np.zeros((s.n, 3))
    v = np.zeros((s.n, 3))
    x[d.tags_local - 1] = got["x"]
    v[d.tags_local - 1] = got["v"]
    st = ctx.L.mdp_nhc_state(ctx.h, capi._dp(np.zeros(capi.NHC_STATE_LEN)))
    assert st != 0                                  # the thermostat is off
    for step in range(1, 101):
        d.step(0, 0, rebuild="auto", defer_final=step < 100)
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    xd = np.zeros((s.n, 3))
    xd[d.tags_local - 1] = got["x"]
    ctx.close()
    # the host: NVE from the state at the switch
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


def test_nhc_off_before_any_step_is_the_nve_code_bit_for_bit():
    """a context whose thermostat was set up and switched off runs the NVE kernels: bit-identical to one that never had it"""
    s, v0 = _rebomos()

    def nve(thermostat_first):
        c = capi.Context(0)
        p = capi.read_rebomos_file(POT_REBOMOS)
        c.rebomos_set_params(p)
        dd = resident.DeviceDomain(c, capi.STYLE_REBOMOS, s, 3.0 * p.rcmax[0][0] + 2.0, 2.0, [0, 0, 1], v0=v0.copy())
        if thermostat_first:
            dd.thermostat(300.0, 300.0, TDAMP)
            dd.thermostat_off()
        dd.compute(1, 0)
        for step in range(1, 101):
            dd.step(0, 0, rebuild="auto", defer_final=step < 100)
        g = c.md_download(dd.nlocal, want=("x", "v"))
        xo = np.zeros((s.n, 3))
        vo = np.zeros((s.n, 3))
        xo[dd.tags_local - 1] = g["x"]
        vo[dd.tags_local - 1] = g["v"]
        c.close()
        return xo, vo

    xa, va = nve(False)
    xb, vb = nve(True)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)


def test_several_ranks_refuse_the_thermostat_in_either_order():
    s, v0 = _rebomos()
    p = capi.read_rebomos_file(POT_REBOMOS)
    cutghost = 3.0 * p.rcmax[0][0] + 2.0
    for thermostat_first in (True, False):
        c = capi.Context(0)
        c.rebomos_set_params(p)
        resident.DeviceDomain(c, capi.STYLE_REBOMOS, s, cutghost, 2.0, [0, 0, 1], v0=v0.copy())
        if thermostat_first:
            c.nhc_setup(300.0, 300.0, 0.1, 3 * s.n - 3)
            with pytest.raises(capi.MdpError, match="one rank only"):
                c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
        else:
            c.dd_setup(s.box, (2, 1, 1), 0, cutghost)
            with pytest.raises(capi.MdpError, match="one rank only"):
                c.nhc_setup(300.0, 300.0, 0.1, 3 * s.n - 3)
        c.close()


def test_c_abi_refusals():
    c = capi.Context(0)
    for kw in ({"t_start": 0.0}, {"t_stop": -1.0}, {"t_period": 0.0}, {"tchain": 0}, {"tchain": 9}, {"tloop": 0}):
        args = {"t_start": 300.0, "t_stop": 300.0, "t_period": 0.1, "tchain": 3, "tloop": 1}
        args.update(kw)
        with pytest.raises(capi.MdpError):
            c.nhc_setup(args["t_start"], args["t_stop"], args["t_period"], 30.0, tchain=args["tchain"], tloop=args["tloop"])
    with pytest.raises(capi.MdpError, match="mdp_nhc_setup not called"):
        c.nhc_run(0, 10)
    c.close()
