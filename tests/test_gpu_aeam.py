"""GPU parity: AEAM through the C-ABI against the CPU oracle on the same inputs (host mode, i.e.
the two halves a LAMMPS PairAEAM::compute() would call around its forward_comm, and resident mode).
Tolerances: forces 1e-9 eV/A, per-atom energy 1e-9 eV, PE 1e-11 rel, virial 1e-9 rel.
(The oracle itself is unpinned by the reference -- see oracle/aeam_oracle.c.)"""
import numpy as np
import pytest

from conftest import POT_AEAM
from lammps_plugins_amd.host import capi, resident, system as S
import aeam_five
import hostplan
import mdref
import oracle_bindings as ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(oracle):
    return oracle.aeam_pot(POT_AEAM)


@pytest.fixture(scope="module")
def pot():
    af = capi.AeamFile(POT_AEAM)
    return af, af.build()


def test_product_tables_equal_oracle_tables(oracle, T, pot):
    """the product's own parser/spline builder (csrc/potfile.cpp) against the oracle's, bit for bit"""
    af, tabs = pot
    fr, rh, z2 = oracle.aeam_splines(T)
    assert af.elements == ["Al", "Si"] and (af.nnonangular, af.nangular) == (1, 1)
    for mine, n, ref in ((tabs.frho_spline, tabs.nfrho * (tabs.nrhomax + 1) * 7, fr),
                         (tabs.rhor_spline, tabs.nrhor * (tabs.nrmax + 1) * 7, rh),
                         (tabs.z2r_spline, tabs.nz2r * (tabs.nrmax + 1) * 7, z2)):
        a = np.ctypeslib.as_array(mine, shape=(n,))
        assert np.array_equal(a, ref.ravel())


def _host_mode(ctx, eng, x):
    xa = eng.all_positions(x)
    nall, nloc = len(xa), eng.nlocal
    ctx.set_atoms_host(nloc, xa, eng.type_all, eng.tag_all, 2, map_=None)
    ctx.set_neighbors_csr_host(eng.nn, eng.off, eng.nb, 1.0)
    d = ctx.aeam_density_host(nloc, eflag=3)
    fp_all = np.concatenate([d["fp"], d["fp"][eng.owner]])          # forward_comm on one periodic rank
    r = ctx.aeam_force_host(nall, nloc, fp_all, eflag=3, vflag=5)
    va = r["vatom"][:nloc].copy()
    np.add.at(va, eng.owner, r["vatom"][nloc:])                      # reverse comm of vatom on one periodic rank
    return dict(f=ob.fold_ghost_forces(r["f"], eng.owner, nloc), eng=d["eng"] + r["eng"], virial=r["virial"],
                eatom=d["eatom"] + r["eatom"], rho=d["rho"], vatom=va)


@pytest.mark.parametrize("ncell,frac,amp", [(5, 0.08, 0.075), (6, 0.0075, 0.05), (4, 0.5, 0.1), (4, 0.0, 0.1)])
def test_host_mode_matches_oracle(oracle, T, pot, ncell, frac, amp):
    """Al-Al, Al-Si, Si-Al, Si-Si pairs and angular triplets with mixed k types"""
    ctx = capi.Context(0)
    ctx.aeam_set_tables(pot[1])
    s = S.jitter(S.fcc_cell(4.045, ncell, frac_type2=frac, seed=99), amp, seed=100)
    eng = mdref.AeamCPU(oracle, T, s)
    g = _host_mode(ctx, eng, s.x)
    o = eng.compute(s.x)
    assert np.abs(g["rho"] - o["rho"][:s.n]).max() < 1e-11
    assert np.abs(g["f"] - o["f_owned"]).max() < 1e-9
    assert g["eng"] == pytest.approx(o["eng"], rel=1e-11)
    assert np.abs(g["eatom"] - o["eatom"][:s.n]).max() < 1e-9
    assert np.allclose(g["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
    # per-atom virial: ev_tally halves + ev_tally3 thirds (pair_aeam.cpp:393,472), folded onto owners
    vo = o["vatom"][:s.n].copy()
    np.add.at(vo, eng.owner, o["vatom"][s.n:])
    assert np.abs(g["vatom"] - vo).max() < 1e-9 * max(1.0, np.abs(vo).max())
    ctx.close()


def _host_mode_device_lists(ctx, eng, x, ntypes=2):
    """the drop-in path of the aeam plugin: the host reports its skin, its list is only CHECKED
    (mdp_aeam_check_host_list); bins, tile lists and the angular centres' rows are built on the device from the
    positions, the device keeps a Hilbert-sorted copy of the atoms and returns everything in the host's order"""
    xa = eng.all_positions(x)
    nall, nloc = len(xa), eng.nlocal
    ctx.aeam_device_lists(True)
    ctx.set_atoms_host(nloc, xa, eng.type_all, eng.tag_all, ntypes, map_=None)
    ctx.set_skin(1.0)
    rows = [np.ascontiguousarray(eng.nb[eng.off[i]:eng.off[i] + eng.nn[i]], dtype=np.int32) for i in range(nall)]
    ctx.aeam_check_host_list(np.arange(nloc, dtype=np.int32), eng.nn, rows, 1.0)
    d = ctx.aeam_density_host(nloc, eflag=3)
    fp_all = np.concatenate([d["fp"], d["fp"][eng.owner]])          # forward_comm on one periodic rank
    r = ctx.aeam_force_host(nall, nloc, fp_all, eflag=3, vflag=5)
    va = r["vatom"][:nloc].copy()
    np.add.at(va, eng.owner, r["vatom"][nloc:])
    return dict(f=ob.fold_ghost_forces(r["f"], eng.owner, nloc), eng=d["eng"] + r["eng"], virial=r["virial"],
                eatom=d["eatom"] + r["eatom"], rho=d["rho"], vatom=va, rows=rows)


@pytest.mark.parametrize("ncell,frac,amp", [(5, 0.08, 0.075), (6, 0.0075, 0.05), (4, 0.5, 0.1)])
def test_host_mode_with_device_lists_matches_oracle(oracle, T, pot, ncell, frac, amp):
    ctx = capi.Context(0)
    ctx.aeam_set_tables(pot[1])
    s = S.jitter(S.fcc_cell(4.045, ncell, frac_type2=frac, seed=99), amp, seed=100)
    eng = mdref.AeamCPU(oracle, T, s)
    g = _host_mode_device_lists(ctx, eng, s.x)
    o = eng.compute(s.x)
    assert np.abs(g["rho"] - o["rho"][:s.n]).max() < 1e-11
    assert np.abs(g["f"] - o["f_owned"]).max() < 1e-9
    assert g["eng"] == pytest.approx(o["eng"], rel=1e-11)
    assert np.abs(g["eatom"] - o["eatom"][:s.n]).max() < 1e-9
    assert np.allclose(g["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
    vo = o["vatom"][:s.n].copy()
    np.add.at(vo, eng.owner, o["vatom"][s.n:])
    assert np.abs(g["vatom"] - vo).max() < 1e-9 * max(1.0, np.abs(vo).max())
    # force-only call with moved positions (between two reneighborings of the host), again against the oracle
    x2 = s.x + 0.02 * np.random.default_rng(3).standard_normal(s.x.shape)
    xa2 = eng.all_positions(x2)
    ctx.set_positions_host(xa2)
    d = ctx.aeam_density_host(eng.nlocal, eflag=0)
    r = ctx.aeam_force_host(len(xa2), eng.nlocal, np.concatenate([d["fp"], d["fp"][eng.owner]]), eflag=0, vflag=0)
    o2 = eng.compute(x2)
    assert np.abs(ob.fold_ghost_forces(r["f"], eng.owner, eng.nlocal) - o2["f_owned"]).max() < 1e-9
    # a host list with an excluded pair is refused; so is handing the list over in this mode
    nn2 = eng.nn.copy()
    nn2[3] -= 1
    with pytest.raises(capi.MdpError) as e:
        ctx.aeam_check_host_list(np.arange(eng.nlocal, dtype=np.int32), nn2, g["rows"], 1.0)
    assert "not the plain geometric list" in str(e.value)
    with pytest.raises(capi.MdpError):
        ctx.set_neighbors_csr_host(eng.nn, eng.off, eng.nb, 1.0)
    ctx.close()


def test_resident_mode_matches_oracle_and_conserves_energy(oracle, T, pot):
    af, tabs = pot
    ctx = capi.Context(0)
    ctx.aeam_set_tables(tabs)
    s = S.jitter(S.fcc_cell(4.045, 6, frac_type2=0.02, seed=5), 0.03, seed=6)
    s.mass[1:3] = af.mass
    cutghost = float(af.cut_table(tabs).max()) + 1.0
    v0 = S.gaussian_velocities(s, 600.0, seed=8)
    d = hostplan.make_domain(ctx, capi.STYLE_AEAM, s, cutghost, 1.0, None, v0=v0)
    d.build_neighbors()
    d.compute(eflag=3, vflag=1)
    t0 = d.thermo()
    got = ctx.md_download(s.n, want=("x", "f", "eatom"))
    x_tag = np.zeros_like(got["x"])
    x_tag[d.tags_local - 1] = got["x"]
    eng = mdref.AeamCPU(oracle, T, S.System(s.box, x_tag, s.type, s.tag, s.mass))
    o = eng.compute(x_tag)
    assert np.abs(got["f"] - o["f_owned"][d.tags_local - 1]).max() < 1e-9
    assert np.abs(got["eatom"] - o["eatom"][:s.n][d.tags_local - 1]).max() < 1e-9
    assert t0["pe"] == pytest.approx(o["eng"], rel=1e-11)
    assert np.allclose(t0["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
    e0 = t0["pe"] + t0["ke"]
    for step in range(1, 201):
        d.ctx.md_initial_integrate()
        if step % 10 == 0 and d.needs_rebuild():           # neigh_modify check yes
            d = hostplan.reneighbor(d, s, cutghost, None)
        d.compute(0, 0)
        d.ctx.md_final_integrate()
    d.compute(eflag=1, vflag=0)
    t1 = d.thermo()
    assert abs(t1["pe"] + t1["ke"] - e0) / s.n < 5e-5   # velocity-Verlet fluctuation at 600 K, dt = 1 fs
    assert d.builds >= 2                                  # hot Al crosses skin/2 = 0.5 A within 200 steps
    ctx.close()


@pytest.mark.parametrize("frac,amp", [(0.02, 0.03), (0.30, 0.05), (0.0, 0.02)])
def test_resident_force_only_step_matches_oracle(oracle, T, pot, frac, amp):
    """Force-only computes in resident mode take the tile-list kernels (aeam_tile_density/force_kernel); steps that
    tally energy or virial take the CSR kernels.  Both must give the oracle's forces: dilute Si (the shipped
    sample), an Si-rich alloy (type-1 row segments and different-element visits everywhere) and pure Al."""
    af, tabs = pot
    ctx = capi.Context(0)
    ctx.aeam_set_tables(tabs)
    s = S.jitter(S.fcc_cell(4.045, 6, frac_type2=frac, seed=11), amp, seed=12)
    s.mass[1:3] = af.mass
    cutghost = float(af.cut_table(tabs).max()) + 1.0
    d = hostplan.make_domain(ctx, capi.STYLE_AEAM, s, cutghost, 1.0, None)
    d.build_neighbors()
    d.compute(eflag=0, vflag=0)                       # tile kernels
    got = ctx.md_download(s.n, want=("x", "f"))
    f_tile = got["f"].copy()
    d.compute(eflag=3, vflag=1)                       # CSR kernels on the same positions
    f_csr = ctx.md_download(s.n, want=("f",))["f"]
    x_tag = np.zeros_like(got["x"])
    x_tag[d.tags_local - 1] = got["x"]
    eng = mdref.AeamCPU(oracle, T, S.System(s.box, x_tag, s.type, s.tag, s.mass))
    o = eng.compute(x_tag)
    ref = o["f_owned"][d.tags_local - 1]
    assert np.abs(f_tile - ref).max() < 1e-9
    assert np.abs(f_csr - ref).max() < 1e-9
    ctx.close()


@pytest.mark.parametrize("env", [
    {"MDP_AEAM_PERSIST": "0"},                                  # gather tile kernels (spline rows from global memory)
    {"MDP_AEAM_PERSIST": "1"},                                  # persistent density kernel, table window in LDS
    {"MDP_AEAM_PERSIST": "1", "MDP_AEAM_PT_NSUB": "4"},         # narrower window, more sub-blocks
    {"MDP_AEAM_PERSIST": "1", "MDP_AEAM_PT_NSUB": "2"},         # widest window, two sub-blocks
    {},                                                         # the library's own choice
])
def test_tile_kernel_variants_match_oracle(oracle, T, pot, env, monkeypatch):
    """Every variant of the two-type tile kernels on a compressed, strongly jittered alloy: 8 % Si puts type-1
    segments and different-element visits (global-memory rows) into every tile, the compression puts pairs
    below the LDS window of the persistent kernels (rows read from global memory in their cold pass), and the
    energy/virial step runs the tallying variants.  All against the CPU oracle."""
    for k in ("MDP_AEAM_PERSIST", "MDP_AEAM_PT_NSUB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    af, tabs = pot
    ctx = capi.Context(0)
    ctx.aeam_set_tables(tabs)
    s = S.jitter(S.fcc_cell(3.55, 6, frac_type2=0.08, seed=21), 0.12, seed=22)   # nearest neighbours at 2.5 A +- 0.3
    s.mass[1:3] = af.mass
    cutghost = float(af.cut_table(tabs).max()) + 1.0
    d = hostplan.make_domain(ctx, capi.STYLE_AEAM, s, cutghost, 1.0, None)
    d.build_neighbors()
    d.compute(eflag=0, vflag=0)
    got = ctx.md_download(s.n, want=("x", "f"))
    f_only = got["f"].copy()
    d.compute(eflag=3, vflag=1)                       # tallying variants of the same kernels
    t = d.thermo()
    got_ev = ctx.md_download(s.n, want=("f", "eatom"))
    x_tag = np.zeros_like(got["x"])
    x_tag[d.tags_local - 1] = got["x"]
    eng = mdref.AeamCPU(oracle, T, S.System(s.box, x_tag, s.type, s.tag, s.mass))
    o = eng.compute(x_tag)
    ref = o["f_owned"][d.tags_local - 1]
    r_min = min(np.linalg.norm(x_tag[i] - x_tag[j]) for i in range(0, 40) for j in range(s.n) if i != j)
    assert r_min < 2.6                                # the point of the compression (window of 4 sub-blocks: r >= 2.5 A)
    assert np.abs(f_only - ref).max() < 2e-9
    assert np.abs(got_ev["f"] - ref).max() < 2e-9
    assert np.abs(got_ev["eatom"] - o["eatom"][:s.n][d.tags_local - 1]).max() < 1e-9
    assert t["pe"] == pytest.approx(o["eng"], rel=1e-11)
    assert np.allclose(t["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
    ctx.close()


@pytest.mark.parametrize("cluster", ["2", "1"])
def test_tile_rows_as_found_match_the_sorted_ones(pot, cluster, monkeypatch):
    """The style's tile rows (mdp_tile_lists_build) with MDP_TILE_SORT=0 -- the unions as the scan found them, rows filled
    by tile_fill_kernel -- against the default, which sorts the unions and fills the rows in one launch: a force-only
    and a tallying compute on 500 atoms (250 two-atom clusters: the last tile is not full), both tile layouts."""
    monkeypatch.setenv("MDP_AEAM_CLUSTER", cluster)
    af, tabs = pot
    s = S.jitter(S.fcc_cell(4.045, 5, frac_type2=0.1, seed=41), 0.06, seed=42)
    s.mass[1:3] = af.mass
    ntile = (s.n // int(cluster) + 15) // 16
    res = []
    for sort in ("1", "0"):
        monkeypatch.setenv("MDP_TILE_SORT", sort)
        ctx = capi.Context(0)
        ctx.aeam_set_tables(tabs)
        d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, s, float(af.cut_table(tabs).max()) + 1.0, 1.0, None)
        d.compute(0, 0)
        f_only = ctx.md_download(d.nlocal, want=("f",))["f"]
        d.compute(3, 1)
        th = d.thermo()
        got = ctx.md_download(d.nlocal, want=("f", "eatom"))
        nu = ctx.md_download_int("tile_nu", d.nlocal)[:2 * ntile]    # (refused unless the tile rows were built)
        order = np.argsort(d.tags_local)
        ctx.close()
        res.append((f_only[order], got["f"][order], got["eatom"][order], th, nu))
    a, b = res
    assert np.array_equal(a[4], b[4]) and a[4][::2].min() > 0    # the same unions, in another order
    assert np.abs(b[0] - a[0]).max() < 1e-9
    assert np.abs(b[1] - a[1]).max() < 1e-9
    assert np.abs(b[2] - a[2]).max() < 1e-9
    assert b[3]["pe"] == pytest.approx(a[3]["pe"], rel=1e-11)
    assert np.allclose(b[3]["virial"], a[3]["virial"], rtol=1e-9, atol=1e-7)


@pytest.mark.parametrize("nmetal,nang", [(3, 2), (7, 5)])
def test_host_mode_with_device_lists_more_types(oracle, tmp_path, nmetal, nang):
    """the same drop-in path with five atom types (three metals, two angular: tile lists with per-entry types in
    host mode) and with twelve (beyond the kernel-argument parameter block: generic kernels over device-built CSR
    lists), everything against the oracle on the same file"""
    path = str(tmp_path / "n.aeam")
    nt = nmetal + nang
    aeam_five.write_relabelled_file(path, POT_AEAM, [0] * nmetal + [1] * nang, ["E%d" % k for k in range(nt)])
    af5 = capi.AeamFile(path)
    T5 = oracle.aeam_pot(path)
    s2 = S.jitter(S.fcc_cell(4.045, 5, frac_type2=0.08, seed=99), 0.075, seed=100)
    rng = np.random.default_rng(7)
    t5 = np.where(s2.type == 1, rng.integers(1, nmetal + 1, s2.n), rng.integers(nmetal + 1, nt + 1, s2.n)).astype(np.int32)
    s5 = S.System(s2.box, s2.x.copy(), t5, s2.tag.copy(), np.array([0.0] + list(af5.mass)))
    eng = mdref.AeamCPU(oracle, T5, s5)
    ctx = capi.Context(0)
    ctx.aeam_set_tables(af5.build())
    g = _host_mode_device_lists(ctx, eng, s5.x, ntypes=nt)
    o = eng.compute(s5.x)
    assert np.abs(g["rho"] - o["rho"][:s5.n]).max() < 1e-11
    assert np.abs(g["f"] - o["f_owned"]).max() < 1e-9
    assert g["eng"] == pytest.approx(o["eng"], rel=1e-11)
    assert np.abs(g["eatom"] - o["eatom"][:s5.n]).max() < 1e-9
    assert np.allclose(g["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
    x2 = s5.x + 0.02 * np.random.default_rng(3).standard_normal(s5.x.shape)
    xa2 = eng.all_positions(x2)
    ctx.set_positions_host(xa2)
    d = ctx.aeam_density_host(eng.nlocal, eflag=0)
    r = ctx.aeam_force_host(len(xa2), eng.nlocal, np.concatenate([d["fp"], d["fp"][eng.owner]]), eflag=0, vflag=0)
    o2 = eng.compute(x2)
    assert np.abs(ob.fold_ghost_forces(r["f"], eng.owner, eng.nlocal) - o2["f_owned"]).max() < 1e-9
    ctx.close()


def _five_element_file(path):
    aeam_five.write_five_element_file(path, POT_AEAM)


@pytest.mark.parametrize("tiles", [True, False])
def test_five_atom_types_size_everything_from_the_file(oracle, tmp_path, tiles, monkeypatch):
    """The reference sizes its tables from the potential file (pair_aeam.cpp:752-872); the bundled file has two
    elements.  Five types (three metals, two angular) built from the same functions: the device result equals the
    oracle's for the five-element file AND the two-type AlSi system's, atom for atom -- through the tile kernels
    (two list segments: type 0 | the other four, the entry's own type and the 25 parameter sets read from LDS) on
    force-only and on tallying steps, and through the CSR kernels (MDP_AEAM_TILE=0)."""
    if not tiles:
        monkeypatch.setenv("MDP_AEAM_TILE", "0")
    path = str(tmp_path / "five.aeam")
    _five_element_file(path)
    s2 = S.jitter(S.fcc_cell(4.045, 6, frac_type2=0.08, seed=11), 0.06, seed=12)
    rng = np.random.default_rng(3)
    t5 = np.where(s2.type == 1, rng.integers(1, 4, s2.n), rng.integers(4, 6, s2.n)).astype(np.int32)
    assert set(t5.tolist()) == {1, 2, 3, 4, 5}
    af5 = capi.AeamFile(path)
    assert af5.nelements == 5 and af5.nnonangular == 3 and af5.nangular == 2
    s5 = S.System(s2.box, s2.x.copy(), t5, s2.tag.copy(), np.array([0.0] + list(af5.mass)))
    out = {}
    for tag, (af, s) in {"five": (af5, s5), "two": (capi.AeamFile(POT_AEAM), s2)}.items():
        tabs = af.build()
        ctx = capi.Context(0)
        ctx.aeam_set_tables(tabs)
        s.mass[1:1 + af.nelements] = af.mass
        d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, s, float(af.cut_table(tabs).max()) + 1.0, 1.0, None)
        d.compute(0, 0)                                   # force-only kernels
        f_only = ctx.md_download(d.nlocal, want=("f",))["f"]
        d.compute(3, 1)
        th = d.thermo()
        got = ctx.md_download(d.nlocal, want=("f", "eatom"))
        order = np.argsort(d.tags_local)
        out[tag] = (got["f"][order], got["eatom"][order], th, f_only[order])
        ctx.close()
    f5, e5, th5, fo5 = out["five"]
    f2, e2, th2, fo2 = out["two"]
    assert np.abs(f5 - f2).max() < 1e-10 and np.abs(e5 - e2).max() < 1e-10
    assert np.abs(fo5 - fo2).max() < 1e-10
    assert th5["pe"] == pytest.approx(th2["pe"], rel=1e-12)
    T5 = oracle.aeam_pot(path)
    xw = S.wrap(s5.box, s5.x)
    o = mdref.AeamCPU(oracle, T5, S.System(s5.box, xw, s5.type, s5.tag, s5.mass)).compute(xw)
    assert np.abs(f5 - o["f_owned"]).max() < 1e-9
    assert np.abs(fo5 - o["f_owned"]).max() < 1e-9
    assert th5["pe"] == pytest.approx(o["eng"], rel=1e-11)


def test_five_atom_types_hot_run_equals_the_two_type_run(tmp_path):
    """60 hot NVE steps (pruned rows, reneighborings on the device) of the five-type system and of the two-type
    system it is a relabelling of: same functions, same masses per class -- the trajectories agree to rounding.  The
    five-type run walks the tile lists with per-entry types, the two-type run the specialised kernels (persistent
    density kernel included)."""
    path = str(tmp_path / "five.aeam")
    _five_element_file(path)
    s2 = S.jitter(S.fcc_cell(4.045, 8, frac_type2=0.05, seed=31), 0.02, seed=32)
    rng = np.random.default_rng(5)
    t5 = np.where(s2.type == 1, rng.integers(1, 4, s2.n), rng.integers(4, 6, s2.n)).astype(np.int32)
    af5 = capi.AeamFile(path)
    s5 = S.System(s2.box, s2.x.copy(), t5, s2.tag.copy(), np.array([0.0] + list(af5.mass)))
    v0 = S.gaussian_velocities(s2, 800.0, seed=33)
    res = {}
    for tag, (af, s) in {"five": (af5, s5), "two": (capi.AeamFile(POT_AEAM), s2)}.items():
        tabs = af.build()
        ctx = capi.Context(0)
        ctx.aeam_set_tables(tabs)
        s.mass[1:1 + af.nelements] = af.mass
        d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, s, float(af.cut_table(tabs).max()) + 1.0, 1.0, None, v0=v0)
        d.compute(0, 0)
        for step in range(60):
            d.step(0, 0, rebuild="auto")
        got = ctx.md_download(d.nlocal, want=("x", "f"))
        order = np.argsort(d.tags_local)
        res[tag] = (got["x"][order], got["f"][order], d.builds, ctx.md_prune_stats())
        ctx.close()
    x5, f5, b5, p5 = res["five"]
    x2, f2, b2, p2 = res["two"]
    assert p5["prunings"] >= 1 and p2["prunings"] >= 1
    dx = x5 - x2
    dx -= np.round(dx / np.diag(s2.box.h)) * np.diag(s2.box.h)      # (an atom may have been wrapped in one run only)
    assert np.abs(dx).max() < 1e-9
    assert np.abs(f5 - f2).max() < 1e-7


@pytest.mark.parametrize("cls,names,cluster", [([0], ["Al"], "2"), ([0, 1, 1], ["Al", "Sia", "Sib"], "2"),
                                               ([0, 0, 1], ["Ala", "Alb", "Si"], "1"),
                                               ([0, 0, 0, 0, 1, 1, 1, 1], list("ABCDEFGH"), "2"),
                                               ([0] * 7 + [1] * 5, ["M%d" % k for k in range(7)] + ["X%d" % k for k in range(5)], "2")])
def test_other_type_counts(oracle, tmp_path, cls, names, cluster, monkeypatch):
    """one element (pure metal: the second list segment is empty), three (one metal: the per-entry types are all
    angular), eight (the most whose parameters ride in the kernel arguments: tile kernels) and twelve (beyond: the
    reference sizes everything from the file, pair_aeam.cpp:752-872 -- generic kernels that read the parameters of a
    pair from device memory): a force-only and a tallying compute against the oracle on the same file"""
    monkeypatch.setenv("MDP_AEAM_CLUSTER", cluster)          # (1: one atom per 16-lane group, the other tile layout)
    path = str(tmp_path / "n.aeam")
    aeam_five.write_relabelled_file(path, POT_AEAM, cls, names)
    af = capi.AeamFile(path)
    assert af.nelements == len(cls)
    s2 = S.jitter(S.fcc_cell(4.045, 5, frac_type2=0.1 if 1 in cls else 0.0, seed=41), 0.06, seed=42)
    rng = np.random.default_rng(9)
    metals = [k + 1 for k, c in enumerate(cls) if c == 0]
    angular = [k + 1 for k, c in enumerate(cls) if c == 1] or metals
    tn = np.where(s2.type == 1, rng.choice(metals, s2.n), rng.choice(angular, s2.n)).astype(np.int32)
    sn = S.System(s2.box, s2.x.copy(), tn, s2.tag.copy(), np.array([0.0] + list(af.mass)))
    ctx = capi.Context(0)
    ctx.aeam_set_tables(af.build())
    d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, sn, float(af.cut_table(af.build()).max()) + 1.0, 1.0, None)
    d.compute(0, 0)
    f_only = ctx.md_download(d.nlocal, want=("f",))["f"]
    d.compute(3, 1)
    th = d.thermo()
    got = ctx.md_download(d.nlocal, want=("f", "eatom"))
    order = np.argsort(d.tags_local)
    ctx.close()
    Tn = oracle.aeam_pot(path)
    xw = S.wrap(sn.box, sn.x)
    o = mdref.AeamCPU(oracle, Tn, S.System(sn.box, xw, sn.type, sn.tag, sn.mass)).compute(xw)
    assert np.abs(f_only[order] - o["f_owned"]).max() < 1e-9
    assert np.abs(got["f"][order] - o["f_owned"]).max() < 1e-9
    assert np.abs(got["eatom"][order] - o["eatom"][:sn.n]).max() < 1e-9
    assert th["pe"] == pytest.approx(o["eng"], rel=1e-11)
    assert np.allclose(th["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
