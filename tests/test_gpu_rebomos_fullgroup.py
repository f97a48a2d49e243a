"""GPU parity of the lane-group centre kernel's two pair-loop paths (rebo_centre_kernel):
the full-group path a wave takes when every centre it holds has exactly as many neighbours as its group has lanes, and
the general loops every other wave takes.

The 288-atom cell has 96 owned Mo centres with 12 neighbours each (the ghost Mo atoms that neighbour owned atoms are
centres too: 34 waves of five 12-lane groups in all): whole waves take the full-group path and the wave that holds the
last, single group does not, so both paths run in one launch.  Every case is compared with the CPU oracle under both
settings of MDP_CENTRE_FULL, with all tallies on and force-only; tolerances as in test_gpu_rebomos.py.

Measured on an MI355X (waves on the full-group path, other waves; with MDP_CENTRE_FULL=0 all of them are "other"):
perfect cell (33, 1), jitter 0.05 (33, 1), jitter 0.15 (32, 16: some Mo centres are classed into 16-lane groups), one S
removed (25, 9), compressed (33, 73).  Largest force difference between the two settings: 0 in every case but the
compressed cell (8.9e-16 eV/A)."""
import dataclasses

import numpy as np
import pytest

from conftest import POT_REBOMOS
from lammps_plugins_amd.host import capi, system as S
import mdref
import oracle_bindings

pytestmark = pytest.mark.gpu

F_TOL, E_TOL = 1e-9, 1e-9


@pytest.fixture(scope="module")
def P(oracle):
    return oracle.rebomos_params(POT_REBOMOS)


@pytest.fixture(scope="module")
def ctx(P):
    c = capi.Context(0)
    c.rebomos_set_params(oracle_bindings.product_rebomos_params(P))
    yield c
    c.close()


def _without_atom(s, i):
    keep = np.arange(s.n) != i
    return dataclasses.replace(s, x=s.x[keep], type=s.type[keep], tag=np.arange(1, s.n, dtype=np.int32))


def _perfect():
    return S.rebomos_bulk_cell()


def _one_s_removed():
    s = S.rebomos_bulk_cell()
    return _without_atom(s, int(np.flatnonzero(s.type == 2)[0]))


# (name, system, what the oracle's Mo coordination must be for the path assertions to apply)
CASES = {
    "perfect": (_perfect, "all12"),
    "jitter0.05": (lambda: S.jitter(S.rebomos_bulk_cell(), 0.05, seed=3), "all12"),
    "jitter0.15": (lambda: S.jitter(S.rebomos_bulk_cell(), 0.15, seed=7), "all12"),
    "one_S_removed": (_one_s_removed, "three11"),
    "compressed": (lambda: S.jitter(S.scale(S.rebomos_bulk_cell(), 0.93), 0.10, seed=77), None),
}


def _compare(g, o):
    assert np.abs(g["f"] - o["f_owned"]).max() < F_TOL
    assert g["eng"] == pytest.approx(o["eng"], rel=1e-10)
    assert np.abs(g["eatom"] - o["eatom_owned"]).max() < E_TOL
    assert np.allclose(g["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)


def _run(ctx, eng, x, monkeypatch, full):
    """one list build, then a compute with every tally and a force-only one; (results, force-only forces, wave counts)"""
    monkeypatch.setenv("MDP_CENTRE_FULL", full)
    monkeypatch.setenv("MDP_CENTRE_COUNT", "1")
    xa = eng.all_positions(x)
    ctx.set_atoms_host(eng.nlocal, xa, eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
    ctx.set_neighbors_csr_host(eng.nn, eng.off, eng.nb, 2.0)
    ctx.rebomos_centre_paths(reset=True)
    g = ctx.rebomos_compute_host(eng.nlocal, eflag=3, vflag=1)
    counts = ctx.rebomos_centre_paths(reset=True)
    g0 = ctx.rebomos_compute_host(eng.nlocal, eflag=0, vflag=0)
    counts0 = ctx.rebomos_centre_paths(reset=True)
    assert counts0 == counts
    return {k: np.copy(v) for k, v in g.items()}, np.copy(g0["f"]), counts


@pytest.mark.parametrize("name", list(CASES))
def test_both_paths_match_oracle(ctx, oracle, P, monkeypatch, name):
    make, coordination = CASES[name]
    s = make()
    eng = mdref.RebomosCPU(oracle, P, s)
    o = eng.compute(s.x)
    nn_mo = o["rebo_numneigh"][:eng.nlocal][s.type == 1]
    if coordination == "all12":
        assert (nn_mo == 12).all()            # (the seeds were chosen so: the case cannot pass vacuously)
    elif coordination == "three11":
        assert (nn_mo == 11).sum() == 3 and (nn_mo == 12).sum() == len(nn_mo) - 3

    g_off, f0_off, cnt_off = _run(ctx, eng, s.x, monkeypatch, "0")
    g_on, f0_on, cnt_on = _run(ctx, eng, s.x, monkeypatch, "1")
    print(f"{name}: waves (full-group, general) with MDP_CENTRE_FULL=0: {cnt_off}, =1: {cnt_on}")
    for g, f0 in ((g_off, f0_off), (g_on, f0_on)):
        _compare(g, o)
        assert np.abs(f0 - o["f_owned"]).max() < F_TOL
    dmax = max(np.abs(g_on["f"] - g_off["f"]).max(), np.abs(f0_on - f0_off).max())
    print(f"{name}: largest force difference between the two settings: {dmax:.3e} eV/A")
    assert dmax < F_TOL

    assert cnt_off[0] == 0 and cnt_off[1] > 0
    assert cnt_on[0] + cnt_on[1] == cnt_off[1]
    if coordination == "all12":
        # Mo centres in 12-lane groups, five to a wave: whole waves take the full-group path, the wave that holds the
        # last single group does not
        assert cnt_on[0] > 0 and cnt_on[1] > 0
    elif coordination == "three11":
        # the waves of the three 11-neighbour centres take the general loops, the others the full-group path
        assert cnt_on[0] > 0 and cnt_on[1] > 1
