"""GPU parity for the REBO pair parameters of the centre kernels (rcmax^2, rcmin, 1/(rcmax-rcmin), alpha, A, Q, B, beta),
which a lane picks by its neighbour's element from two scalar candidates of the centre's element (rebomos.hip: PairPar;
the general kernel reads an LDS table at the lane's pair type).

The cells of test_gpu_rebomos.py hardly reach them: in the 288-atom cell scaled by 0.93 / jittered by 0.10 (seed 77) no
Mo-Mo and no Mo-S pair sits in its switching interval, in the cell jittered by 0.15 (seed 5) four Mo-Mo pairs do and no
Mo-S pair, and every Mo centre has its twelve neighbours.  Here one atom in eight of the same two cells changes its
element.  Then every class of centres (the lane-per-centre kernel, the 8-, 12- and 16-lane groups) sees both neighbour
elements inside one lane group and every pair type inside its switching interval:

  cell                      pairs in the switching interval [centre][neighbour]    neighbours per centre
  x 1.0 / 0.15 / seed 5     [[14, 31], [31, 132]]                                  Mo 3-13, S 3-7
  x 0.93 / 0.10 / seed 77   [[120, 179], [179, 704]]                               Mo 9-15, S 6-12

(a census on the CPU from the oracle's neighbour data; the tests assert it before they compare, so that a change of
the recipe cannot empty it unnoticed).  Same host-CSR route and tolerances as test_gpu_rebomos.py."""
import dataclasses

import numpy as np
import pytest

from conftest import POT_REBOMOS
from lammps_plugins_amd.host import capi, system as S
import mdref
import oracle_bindings

pytestmark = pytest.mark.gpu

F_TOL, E_TOL = 1e-9, 1e-9

CELLS = {(1.0, 0.15, 5): [[14, 31], [31, 132]], (0.93, 0.10, 77): [[120, 179], [179, 704]]}


@pytest.fixture(scope="module")
def P(oracle):
    return oracle.rebomos_params(POT_REBOMOS)


@pytest.fixture(scope="module")
def ctx(P):
    c = capi.Context(0)
    c.rebomos_set_params(oracle_bindings.product_rebomos_params(P))
    yield c
    c.close()


def _swapped_cell(fac, amp, seed):
    s = S.jitter(S.scale(S.rebomos_bulk_cell(), fac), amp, seed=seed)
    swap = np.random.default_rng(11).choice(288, 36, replace=False)
    t = s.type.copy()
    t[swap] = 3 - t[swap]
    return dataclasses.replace(s, type=t)


def _census(eng, P, x):
    """ordered pairs (owned centre, listed neighbour) with rcmin < r < rcmax by [centre element][neighbour element]; per
    owned centre the number of neighbours inside rcmax and whether they are of both elements"""
    xa = eng.all_positions(x)
    rcmin = np.array([[P.rcmin[a][b] for b in range(2)] for a in range(2)])
    rcmax = np.array([[P.rcmax[a][b] for b in range(2)] for a in range(2)])
    zone = np.zeros((2, 2), dtype=int)
    coord = np.zeros(eng.nlocal, dtype=int)
    mixed = np.zeros(eng.nlocal, dtype=bool)
    for i in range(eng.nlocal):
        j = eng.nb[eng.off[i]:eng.off[i] + eng.nn[i]]
        r = np.linalg.norm(xa[j] - xa[i], axis=1)
        ei, ej = eng.elem[i], eng.elem[j]
        inside = r < rcmax[ei][ej]
        coord[i] = inside.sum()
        mixed[i] = len(set(ej[inside].tolist())) == 2
        for b in range(2):
            zone[ei, b] += (inside & (r > rcmin[ei][ej]) & (ej == b)).sum()
    return zone, coord, mixed


@pytest.fixture(scope="module")
def cells(oracle, P):
    """each cell once: the system, its engine (ghosts + lists) and the oracle's result with every tally on"""
    out = {}
    for key in CELLS:
        s = _swapped_cell(*key)
        eng = mdref.RebomosCPU(oracle, P, s)
        out[key] = (s, eng, eng.compute(s.x))
    return out


def _gpu_compute(ctx, eng, x, eflag=3, vflag=1):
    ctx.set_atoms_host(eng.nlocal, eng.all_positions(x), eng.type_all, eng.tag_all, 2, map_=[0, 0, 1])
    ctx.set_neighbors_csr_host(eng.nn, eng.off, eng.nb, 2.0)
    return ctx.rebomos_compute_host(eng.nlocal, eflag=eflag, vflag=vflag)


def _compare(g, o):
    assert np.abs(g["f"] - o["f_owned"]).max() < F_TOL
    assert g["eng"] == pytest.approx(o["eng"], rel=1e-10)
    assert np.abs(g["eatom"] - o["eatom_owned"]).max() < E_TOL
    assert np.allclose(g["virial"], o["virial_fdotr"], rtol=1e-9, atol=1e-7)
    assert g["eatom"].sum() == pytest.approx(g["eng"], rel=1e-11)


def _assert_census(P, s, eng, o, want):
    zone, coord, mixed = _census(eng, P, s.x)
    assert (zone > 0).all(), zone                             # every pair type inside its switching interval
    assert zone.tolist() == want
    assert (coord == o["rebo_numneigh"][:eng.nlocal]).all()   # (the oracle's own REBO lists say the same)
    for el in (1, 2):                                         # both neighbour elements around centres of either element
        assert mixed[s.type == el].any()
    return coord, mixed


@pytest.mark.parametrize("key", list(CELLS))
def test_swapped_elements_match_oracle_with_all_tallies(ctx, P, cells, key):
    s, eng, o = cells[key]
    _assert_census(P, s, eng, o, CELLS[key])
    _compare(_gpu_compute(ctx, eng, s.x), o)


@pytest.mark.parametrize("key", list(CELLS))
def test_swapped_elements_per_atom_virial(ctx, P, cells, key):
    """vflag_atom sends every centre through the general kernel, which reads the parameters from its LDS table (centres
    of both elements in one wave); compared as in test_gpu_rebomos.py::test_per_atom_virial_matches_oracle"""
    s, eng, o = cells[key]
    g = _gpu_compute(ctx, eng, s.x, eflag=3, vflag=5)
    va = o["vatom"][:eng.nlocal].copy()
    np.add.at(va, eng.owner, o["vatom"][eng.nlocal:])
    assert np.abs(g["vatom"] - va).max() < 1e-9 * max(1.0, np.abs(va).max())
    assert np.allclose(g["vatom"].sum(axis=0), g["virial"], rtol=1e-9, atol=1e-8)
    _compare(g, o)


@pytest.mark.parametrize("key", list(CELLS))
def test_swapped_elements_force_only(ctx, P, cells, key):
    """eflag = vflag = 0: the kernel variants an MD step runs"""
    s, eng, o = cells[key]
    zone = _census(eng, P, s.x)[0]
    assert (zone > 0).all(), zone
    g = _gpu_compute(ctx, eng, s.x, eflag=0, vflag=0)
    assert g["eng"] == 0.0 and not g["virial"].any() and not g["eatom"].any()
    assert np.abs(g["f"] - o["f_owned"]).max() < F_TOL
