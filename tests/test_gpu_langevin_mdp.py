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
from refloops import host_lgv as _host_lgv, worse
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


def _compare(s, host, dev, xtol=1e-9, etol=1e-9):
    worst_x = worst_e = 0.0
    for step in sorted(host):
        xh, eh = host[step][:2]
        xd, ed = dev[step][:2]
        dx = xd - xh
        dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
        worst_x = max(worst_x, float(np.abs(dx).max()))
        worst_e = worse(worst_e, abs(ed - eh))
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


XTOL, VTOL, ETOL = 1e-9, 2e-8, 1e-8     # the limits of the `langevin` net (tests/nets.py)


def _close(s, x, v, e, ref, what):
    """positions (same atom, possibly another image), velocities and tally against a row (x, tally, v) of _host_lgv"""
    dx = x - ref[0]
    dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
    wx, wv, we = float(np.abs(dx).max()), float(np.abs(v - ref[2]).max()), abs(e - ref[1])
    print(f"{what}: |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps, |dE| {we:.2e} eV (tally {ref[1]:.4g} eV)")
    assert wx < XTOL and wv < VTOL and we < ETOL, (what, wx, wv, we)
    return wx, wv, we


def _by_tag(ctx, d, s):
    got = ctx.md_download(d.nlocal, want=("x", "v"))
    x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
    x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
    return x, v


def test_two_runs_and_a_hold_on_one_context(oracle, capsys):
    """mdp_langevin_run twice on ONE context, then steps beyond the run's last.  Run 1: steps 1 .. 40 over (0, 40), the
    last final half left deferred.  mdp_langevin_run(40, 80) completes it with run 1's force; the tally read then is run
    1's.  Run 2 ramps Tstart -> Tstop again over (40, 80): the setup force at step 40 with phase 1 of the noise, the tally
    restarted at 0.5 E dt; 20 more steps beyond `last` hold Tstop (lgv_target's clamp).  The reference does the same with
    two calls of _host_lgv (setup(0, 40), then setup(40, 80) from the positions and velocities of step 40, run for 60
    steps).  Positions, velocities and tally at 40, 80 and 100 to the net's limits (1e-9 A, 2e-8 A/ps, 1e-8 eV).
    Measured on an MI355X: 7.1e-15 / 1.4e-14 / 2.1e-14 A, 4.4e-13 / 1.1e-12 / 1.4e-12 A/ps, 8.5e-14 / 7.1e-14 / 5.0e-13 eV at
    steps 40 / 80 / 100 (tallies of -72.8, -33.5 and -65.7 eV)."""
    P = oracle.rebomos_params(POT_REBOMOS)
    s, v0 = _rebomos()
    case = CASES["ramp-scale-zero-tally"]
    t0, t1, ratio, zero, tally = case
    make = lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)   # noqa: E731
    ref1 = _host_lgv(make, s, v0, 40, (40,), 50, _lgv(s, case), skin=2.0)
    s40 = S.System(s.box, ref1[40][0], s.type, s.tag, s.mass)
    ref2 = _host_lgv(make, s40, ref1[40][2], 60, (40, 60), 50, _lgv(s, case), first=40, last=80, skin=2.0)
    ctx, d = _domain(capi.STYLE_REBOMOS, s, v0)
    try:
        d.langevin(t0, t1, DAMP, SEED, ratio=ratio, zero=zero, tally=tally, first=0, last=40)
        d.compute(1, 0)
        for step in range(1, 41):
            d.step(0, 0, rebuild="auto", defer_final=True)
        assert d._final_pending
        d.langevin_run(40, 80)            # (the library completes the deferred final half of step 40 itself)
        e = ctx.langevin_tally()
        with capsys.disabled():
            _close(s, *_by_tag(ctx, d, s), e, ref1[40], "step 40 (end of run 1)")
            d.compute(1, 0)                   # Verlet::setup of run 2
            for step in range(41, 101):
                d.step(0, 0, rebuild="auto", defer_final=True)
                if step in (80, 100):
                    e = d.langevin_tally()
                    _close(s, *_by_tag(ctx, d, s), e, ref2[step - 40], f"step {step}")
    finally:
        ctx.close()
    assert abs(ref1[40][1]) > 1e-3 and abs(ref2[60][1]) > 1e-3      # the thermostat exchanged energy in both runs
    # the hold matters: without the clamp the target at step 100 would be Tstart + 1.5 (Tstop - Tstart)
    held = _lgv(s, case)
    held.setup(40, 80)
    assert held.target(100) == t1 != t0 and held.target(60) == 0.5 * (t0 + t1)


def test_a_changed_time_step_rewrites_the_factors(oracle, capsys):
    """Host-linked: 30 steps at 1 fs; then mdp_hnve_setup with 2 fs (it marks the device's velocities stale, so x and v
    come up before it and mdp_hnve_upload_v follows it, as at a host reneighbouring), mdp_langevin_run(30, 60) and 30
    more steps, which must follow the reference built with dt = 0.002: gfactor2 ~ 1 / sqrt(dt) is cached per (dt, ftm2v)
    in lgv_tables and has to be rewritten.  A resident context cannot change its time step through the C-ABI (dt is part
    of mdp_md_config, read by mdp_md_setup alone), so there is no resident twin of this test.
    Measured on an MI355X: 7.1e-15 A, 4.1e-13 A/ps, 3.6e-14 eV at step 30; 1.4e-14 A, 8.5e-13 A/ps, 2.7e-13 eV at step 60."""
    P = oracle.rebomos_params(POT_REBOMOS)
    s, v0 = _rebomos()
    case = CASES["ramp-scale-zero-tally"]
    t0, t1, ratio, zero, tally = case
    make = lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)   # noqa: E731
    ref1 = _host_lgv(make, s, v0, 30, (30,), 50, _lgv(s, case), skin=2.0)
    s30 = S.System(s.box, ref1[30][0], s.type, s.tag, s.mass)
    ref2 = _host_lgv(make, s30, ref1[30][2], 30, (30,), 50, _lgv(s, case, dt=0.002), dt=0.002, first=30, skin=2.0)
    c = capi.Context(0)
    try:
        c.rebomos_set_params(ob.product_rebomos_params(P))
        c.set_box_host(s.box)
        x = S.wrap(s.box, s.x)
        eng = mdref.RebomosCPU(oracle, P, S.System(s.box, x.copy(), s.type, s.tag, s.mass), skin=2.0)
        c.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
        c.set_skin(2.0)
        c.hnve_setup(0.001, S.FTM2V, s.mass)
        c.langevin_setup(t0, t1, DAMP, SEED, s.n, ratio=ratio, zero=zero, tally=tally, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        c.langevin_run(0, 30)
        c.hnve_upload_v(v0)
        c.rebomos_compute_host(eng.nlocal, eflag=0, vflag=0)
        for step in range(1, 31):
            c.hnve_initial()
            c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
            c.hnve_final()
        got = c.hnve_download(s.n, want=("x", "v"))
        with capsys.disabled():
            _close(s, got["x"], got["v"], c.langevin_tally(), ref1[30], "step 30 (1 fs)")
            c.hnve_setup(0.002, S.FTM2V, s.mass)
            c.langevin_run(30, 60)
            c.hnve_upload_v(got["v"])
            c.rebomos_compute_host(eng.nlocal, eflag=0, vflag=0)
            for step in range(31, 61):
                c.hnve_initial()
                c._ck(c.L.mdp_rebomos_compute_host(c.h, 0, 0, None, None, None, None, None))
                c.hnve_final()
            got = c.hnve_download(s.n, want=("x", "v"))
            _close(s, got["x"], got["v"], c.langevin_tally(), ref2[30], "step 60 (2 fs)")
    finally:
        c.close()


@pytest.mark.parametrize("style", ["aeam", "rebomos"])
def test_zero_and_tally_sum_every_partial(style, capsys):
    """More than 256 per-block partials (70 304 alloy atoms, 69 120 of MoS2: mdp_slot_sum_256 makes more than one trip) with
    zero yes, tally yes and a ratio.  No oracle at this size; per step the device's own forces and velocities come down
    after the compute, a final half runs on its own (it writes f + f_L back) and f comes down again: the difference per atom
    must be langevinref's force for those velocities with the mean of the random parts taken by math.fsum, to 1e-12 eV/A
    (the rounding of f + f_L at |f| < 100 eV/A is below 2e-14; that bound on |f| is asserted).  The setup force is added
    in registers and never written back: it is recovered from the velocities around the first initial half,
    f_L = (v' - v) m / dtf - f, whose rounding (|v| < 20 A/ps, m < 100, dtf = 4.8) stays below 1e-13.  The tally after
    step k must be -(e_0 / 2 + e_1 + ... + e_k / 2) dt with e = fsum(f_L . v), to 1e-12 of dt fsum(|f_L . v|) summed over
    the steps so far.  Measured on an MI355X: worst |f_L - reference| 5.3e-15 (alloy) / 8.9e-15 eV/A (MoS2); the tally
    within 2e-18 of its scale."""
    import math
    import test_gpu_nvt_net as NN
    s, v0 = NN._big(style)
    assert s.n > 65536 and -(-s.n // 256) > 256
    ratio, dt, nsteps = {1: 2.0, 2: 0.5}, 0.001, 3
    lg = langevinref.Langevin(300.0, 330.0, DAMP, SEED, s.mass, dt, S.FTM2V, boltz=S.BOLTZ, mvv2e=S.MVV2E, ratio=ratio, zero=True,
                              tally=True)
    lg.setup(0, nsteps)
    dtf = 0.5 * dt * S.FTM2V
    ctx, d = _domain(capi.STYLE_AEAM if style == "aeam" else capi.STYLE_REBOMOS, s, v0)

    def f_l(step, tags, types, v, phase=0):
        fran = lg.random(step, tags, types, phase)
        mean = np.array([math.fsum(fran[:, k]) for k in range(3)]) / s.n
        return lg.g1[types][:, None] * v + fran - mean

    def dot(a, b):
        p = (a * b).ravel()
        return math.fsum(p), math.fsum(np.abs(p))
    try:
        d.langevin(300.0, 330.0, DAMP, SEED, ratio=ratio, zero=True, tally=True, first=0, last=nsteps)
        d.compute(0, 0)
        tags, types = d.tags_local.copy(), ctx.md_download_int("type", d.nlocal).copy()
        m = s.mass[types][:, None]
        worst_f = worst_e = 0.0
        # the setup force: in the first initial half
        a = ctx.md_download(d.nlocal, want=("v", "f"))
        ctx.md_initial_integrate()
        b = ctx.md_download(d.nlocal, want=("v",))
        want = f_l(0, tags, types, a["v"], phase=1)
        assert np.abs(a["f"]).max() < 100.0
        worst_f = worse(worst_f, float(np.abs((b["v"] - a["v"]) * m / dtf - a["f"] - want).max()))
        e0, scale = dot(want, a["v"])
        energy, e_last, scale = 0.5 * e0 * dt, e0, 0.5 * scale * dt
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
            e, ea = dot(want, b["v"])
            energy, e_last, scale = energy + e * dt, e, scale + ea * dt
            got = ctx.langevin_tally()
            worst_e = worse(worst_e, abs(got + (energy - 0.5 * e_last * dt)) / scale)
            assert np.abs(b["v"] - a["v"] - dtf * b["f"] / m).max() < 1e-12   # and the final half used f + f_L
    finally:
        ctx.close()
    with capsys.disabled():
        print(f"{style} {s.n} atoms: worst |f_L - reference| {worst_f:.2e} eV/A, tally {worst_e:.2e} of its scale")
    assert worst_f < 1e-12, worst_f
    assert worst_e < 1e-12, worst_e


def test_migration_keeps_the_noise(oracle, capsys):
    """One `bricks` case of the langevin net (tests/nets.py) written out: 2 x 2 x 2 bricks of a 2 x 2 x 2 MoS2 replica
    (2 304 atoms) with a drift, reneighbourings forced every 5 steps, the run crossing step 2^32.  More than 10 atoms
    change owner between the reads; three of them must follow the reference before and after the change, to the net's
    limits -- the noise is keyed by the tag an atom carries, not by the slot or the rank that holds it.
    Measured on an MI355X: the three atoms (owners 0 0 0 -> 2 2 3) 2.1e-14 A, 7.8e-13 A/ps; all atoms 5.0e-14 A, 2.7e-12 A/ps."""
    import nets
    spec = dict(style="rebomos", path="bricks", size=(2, 2, 2), n=8 * 288, frac=None, tilt=None, skin=2.0, first=2 ** 32 - 20, nsteps=40,
                dt=0.001, damp=DAMP, t0=300.0, t1=900.0, ratio="all", zero=False, tally=False, ranks=8, drift=[60, -45, 30], renb=5,
                seed=7, reads=[(k, k % 10 == 0) for k in range(5, 41, 5)])
    s, v0, safe = nets._lgv_system(spec)
    every = min(spec["renb"], safe)
    P = oracle.rebomos_params(POT_REBOMOS)
    lgv = langevinref.Langevin(spec["t0"], spec["t1"], DAMP, nets.LGV_SEED, s.mass, spec["dt"], S.FTM2V, boltz=S.BOLTZ, mvv2e=S.MVV2E,
                               ratio=nets.LGV_RATIOS["all"])
    host = _host_lgv(lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0), s, v0, 40, dict(spec["reads"]), every, lgv,
                     first=spec["first"], skin=2.0)
    dev, left, once, builds, late = nets._lgv_device(spec, s, v0, 8, every)
    assert once and left > 10, (once, left)
    steps = sorted(dev)
    changed = np.flatnonzero(dev[steps[0]][3] != dev[steps[-1]][3])
    assert len(changed) >= 3
    pick = changed[:3]
    with capsys.disabled():
        for step in steps:
            dx = dev[step][0] - host[step][0]
            dx -= np.round(s.box.x2lamda(dx + s.box.lo)) @ s.box.h.T
            dv = dev[step][1] - host[step][2]
            print(f"step {step}: tags {(pick + 1).tolist()} on ranks {dev[step][3][pick].tolist()}, |dx| {np.abs(dx[pick]).max():.2e} A, "
                  f"|dv| {np.abs(dv[pick]).max():.2e} A/ps; all atoms {np.abs(dx).max():.2e} A, {np.abs(dv).max():.2e} A/ps")
            assert np.abs(dx[pick]).max() < XTOL and np.abs(dv[pick]).max() < VTOL, step
            assert np.abs(dx).max() < XTOL and np.abs(dv).max() < VTOL, step
    assert any(len(set(dev[k][3][a] for k in steps)) > 1 for a in pick)


@pytest.fixture(scope="module")
def native_langevin(tmp_path_factory):
    """the Langevin cases of tests/native_ranks_child.py: rank threads of ONE child process on the library's own transport,
    bound to the RCCL test double (see tests/test_gpu_native_ranks.py)"""
    import json
    import subprocess
    import sys
    import test_gpu_native_ranks as NR
    d = tmp_path_factory.mktemp("native_langevin")
    out, log = d / "results.json", d / "child.log"
    names = [f"langevin_{style}_{world}" for style in ("rebomos", "aeam") for world in (2, 4)]
    with open(log, "w") as fh:
        p = subprocess.run([sys.executable, NR.CHILD, str(out)] + names, env=NR._env(), stdout=fh, stderr=subprocess.STDOUT, timeout=900)
    assert out.exists(), f"the child wrote nothing (exit {p.returncode}); see {log}:\n{log.read_text()[-3000:]}"
    return json.load(open(out))


@pytest.mark.parametrize("style,world", [("rebomos", 2), ("rebomos", 4), ("aeam", 2), ("aeam", 4)])
def test_bricks_on_the_librarys_own_transport_keep_the_thermostat(native_langevin, style, world, capsys):
    """whole steps in mdp_dd_comm_step_begin / _end with the final half of every step but the thermo steps deferred
    (with_final = 1) under a thermostat that heats 300 -> 900 K: per atom the N-rank run ends where the one-rank run
    ends, to the dd net's limits (1e-8 A, 1e-7 A/ps).  Measured on an MI355X: 2.1e-14 A, 1.3e-12 A/ps (REBO-MoS, 4
    reneighbourings), 1.4e-14 A, 3.5e-13 A/ps (alloy, 6), on 2 and 4 ranks alike."""
    r = native_langevin.get(f"langevin_{style}_{world}")
    assert r is not None and "error" not in r, r
    with capsys.disabled():
        print(f"langevin on the library's transport, {style} x {world}: dx {r['dx']:.2e} A, dv {r['dv']:.2e} A/ps, builds {r['builds']}")
    assert r["owned_once"]
    assert r["dx"] < 1e-8 and r["dv"] < 1e-7
    assert len(set(r["builds"])) == 1 and r["builds"][0] >= 3
    assert r["late"] == [0] * world and r["late_one"] == 0
    assert min(r["nrecv"]) > 0


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
