"""GPU: the Nose-Hoover chain thermostat (csrc/nhc.hip) beyond the fixed cases of tests/test_gpu_nvt_mdp.py.

- A randomised net at the fixed seed of tests/nets.py NVT_SUITE (draw_nvt; tests/test_net_draws.py checks its corners):
  chains of 1-8 (8 included, on both paths: eta_dot[M] is read), 1-3 loops, drag, flat or ramped targets, both styles,
  the resident path and, for REBO-MoS, the host-linked one (mdp_hnve_*, host reneighborings), atom counts whose last 256-atom block varies (n % 256 == 1 no cell shape of either style allows), against velocity Verlet plus tests/nhcref.py
  around the ORACLE forces with the tolerances of the fixed cases.
- More than 256 per-block partial sums (above 65 536 atoms the chain kernel's strided sum makes more than one trip):
  the device's temperature must equal 2 KE / ((3N - 3) k_B) of the downloaded velocities (math.fsum) to rel 1e-12, and
  the chain state the reference driven by those temperatures."""
import copy
import math

import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, system as S
import mdref
import nets
import nhcref
import oracle_bindings as ob
import test_gpu_nvt_mdp as NV

pytestmark = pytest.mark.gpu


NSTEPS = 60
NVT_SEED, NVT_CASES = nets.NVT_SUITE


def _hostlinked(oracle, s, v0, case, nsteps, every, rebuild_every):
    """the loop of test_gpu_nvt_mdp.test_hostlinked_nvt_follows_the_host_chain: mdp_hnve_* with the thermostat, host
    reneighborings every rebuild_every steps"""
    tchain, tloop, drag, t0, t1 = case
    P = oracle.rebomos_params(POT_REBOMOS)
    c = capi.Context(0)
    try:
        c.rebomos_set_params(ob.product_rebomos_params(P))
        c.set_box_host(s.box)
        x = S.wrap(s.box, s.x)
        eng = mdref.RebomosCPU(oracle, P, S.System(s.box, x.copy(), s.type, s.tag, s.mass), skin=2.0)
        c.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
        assert c.host_ghosts_derived()
        c.set_skin(2.0)
        c.hnve_setup(0.001, S.FTM2V, s.mass)
        c.nhc_setup(t0, t1, NV.TDAMP, 3 * s.n - 3, tchain=tchain, tloop=tloop, drag=drag, boltz=S.BOLTZ, mvv2e=S.MVV2E)
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
        return dev
    finally:
        c.close()


@pytest.mark.parametrize("spec", nets.nvt_cases(NVT_SEED, NVT_CASES),
                         ids=[f"seed{NVT_SEED}-case{k}-{s['style']}-{s['path']}-n{s['n']}-chain{s['tchain']}-loop{s['tloop']}-drag{s['drag']}-T{s['t0']:.0f}-{s['t1']:.0f}"
                              for k, s in enumerate(nets.nvt_cases(NVT_SEED, NVT_CASES))])
def test_nvt_net(oracle, spec):
    if spec["style"] == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), spec["size"])
        P = oracle.rebomos_params(POT_REBOMOS)
        make, skin, rebuild_every, st = (lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0)), 2.0, 50, capi.STYLE_REBOMOS
    else:
        af = capi.AeamFile(POT_AEAM)
        s = S.fcc_cell(4.045, spec["size"], frac_type2=0.03, seed=spec["seed"])
        s.mass[1:3] = af.mass[:2]
        T = oracle.aeam_pot(POT_AEAM)
        make, skin, rebuild_every, st = (lambda sy: mdref.AeamCPU(oracle, T, sy, skin=1.0)), 1.0, 25, capi.STYLE_AEAM
    assert s.n == spec["n"]
    v0 = S.gaussian_velocities(s, spec["t0"], seed=spec["seed"] + 1)
    case = (spec["tchain"], spec["tloop"], spec["drag"], spec["t0"], spec["t1"])
    nhc = nhcref.NHC(spec["t0"], spec["t1"], NV.TDAMP, 3 * s.n - 3, 0.001, tchain=spec["tchain"], tloop=spec["tloop"],
                     drag=spec["drag"], boltz=S.BOLTZ, mvv2e=S.MVV2E)
    host = NV._host_nvt(make, s, v0, NSTEPS, 15, skin, rebuild_every, nhc)
    if spec["path"] == "hostlinked":
        dev = _hostlinked(oracle, s, v0, case, NSTEPS, 15, rebuild_every)
    else:
        dev, d, ctx = NV._resident(st, s, v0, case, nsteps=NSTEPS, every=15)
        ctx.close()
    NV._compare(s, host, {k: v[:3] for k, v in dev.items()})


def _big(style):
    if style == "aeam":
        af = capi.AeamFile(POT_AEAM)
        s = S.fcc_cell(4.045, 26, frac_type2=0.03, seed=3)            # 70 304 atoms
        s.mass[1:3] = af.mass[:2]
    else:
        s = S.replicate(S.rebomos_bulk_cell(), (8, 6, 5))             # 69 120 atoms
    return s, S.gaussian_velocities(s, 300.0, seed=4)


@pytest.mark.parametrize("style", ["aeam", "rebomos"])
def test_chain_temperature_sums_every_partial(style):
    s, v0 = _big(style)
    assert s.n > 65536 and -(-s.n // 256) > 256
    tchain, tloop, drag, nsteps = 8, 2, 0.2, 4
    dev_style = capi.STYLE_AEAM if style == "aeam" else capi.STYLE_REBOMOS
    ctx = capi.Context(0)
    if style == "aeam":
        af = capi.AeamFile(POT_AEAM)
        tabs = af.build()
        ctx.aeam_set_tables(tabs)
        skin, cutghost, map_ = 1.0, float(af.cut_table(tabs).max()) + 1.0, None
    else:
        p = capi.read_rebomos_file(POT_REBOMOS)
        ctx.rebomos_set_params(p)
        skin, cutghost, map_ = 2.0, 3.0 * p.rcmax[0][0] + 2.0, [0, 0, 1]
    from lammps_plugins_amd.host import resident
    try:
        d = resident.DeviceDomain(ctx, dev_style, s, cutghost, skin, map_, v0=v0)
        d.thermostat(300.0, 330.0, 0.02, tchain=tchain, tloop=tloop, drag=drag, first=0, last=nsteps)
        nf = 3.0 * s.n - 3.0
        ref = nhcref.NHC(300.0, 330.0, 0.02, nf, 0.001, tchain=tchain, tloop=tloop, drag=drag, boltz=S.BOLTZ, mvv2e=S.MVV2E)

        def temp_of(v, tags):
            m = s.mass[s.type[tags - 1]]
            ke = 0.5 * S.MVV2E * math.fsum((m[:, None] * v * v).ravel())
            return 2.0 * ke / (nf * S.BOLTZ)

        got = ctx.md_download(d.nlocal, want=("v",))
        ref.setup(np.zeros((1, 3)), np.ones(1), 0, nsteps)       # (the masses and targets; T of the setup, below)
        ref.T = temp_of(got["v"], d.tags_local)
        d.compute(0, 0)
        for step in range(1, nsteps + 1):
            ref.begin_step(step)
            ref.half()
            d.step(0, 0, rebuild="auto")
            st = d.thermostat_state()
            v = ctx.md_download(d.nlocal, want=("v",))["v"]
            # the device's T is that of the velocities after the final scaling (the chain carries T *= s^2)
            assert st["temp"] == pytest.approx(temp_of(v, d.tags_local), rel=1e-12), step
            # the reference's final half from the temperature before the scaling: T_before = T_after / S(T_before)^2
            t_before, before = st["temp"], ref
            for _ in range(8):
                ref = copy.deepcopy(before)
                factor = ref.half(t_before)
                t_before = st["temp"] / (factor * factor)
            assert ref.T == pytest.approx(st["temp"], rel=1e-12)
            np.testing.assert_allclose(st["eta"][:tchain], ref.eta, rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(st["eta_dot"][:tchain], ref.eta_dot[:tchain], rtol=1e-12, atol=1e-300)
            assert st["energy"] == pytest.approx(ref.energy(), rel=1e-12)
    finally:
        ctx.close()
