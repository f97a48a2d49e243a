"""GPU: `compute rdf/mdp` through `plugin load` + `run` in the mini-host -- the drifting perfect fcc crystal of
tests/test_gpu_msd_mdp_plugin.py, whose coordination numbers are the shell sums 12, 18, 42, 54, 78 on 1, 2 and 4 ranks;
two computes with different Nbin on one run; the hot alloy with two pair columns and a group on 1 and 2 ranks; and the
refusals that need a run to be seen."""
import math
import re

import numpy as np
import pytest

from test_plugin_boundary import _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env
from test_gpu_msd_mdp_plugin import DRIFT

pytestmark = pytest.mark.gpu

A = 4.045
CUTFORCE = 6.5                                  # AlSi.aeam: the pair style's cutforce, the default cutoff of the compute
SHELLS = [(A * math.sqrt(k / 2.0), c) for k, c in ((1, 12), (2, 18), (3, 42), (4, 54), (5, 78))]   # radius, atoms within it
HEADER = DRIFT.replace("plugin load msdmdpplugin.so", "plugin load rdfmdpplugin.so")


def _shell_bins(nbin):
    """the bin of every fcc shell under cutforce, each at least a quarter of a bin from both its edges: a 0 K lattice is read
    here, and no rounding of a distance may decide its bin"""
    at = [r * nbin / CUTFORCE for r, _ in SHELLS]
    assert all(r < CUTFORCE for r, _ in SHELLS) and A * math.sqrt(3.0) > CUTFORCE
    assert all(0.25 <= t % 1.0 <= 0.75 for t in at), at
    return [int(t) for t in at]


NA, NB = 28, 44
BINS_A, BINS_B = _shell_bins(NA), _shell_bins(NB)


@pytest.fixture(scope="module")
def drift_runs():
    """the crystal going twice through the box in 200 steps, with compute a (28 bins) and compute b (44 bins) on the same
    run, on 1, 2 and 4 ranks: step, g of all 28 bins of a, then per shell the coordination of a and of b at the bin just
    past the shell (the last shell sits in the last bin of both: read there)"""
    past = lambda b, n: min(b + 1, n - 1) + 1                                # 1-based row just past the shell's bin
    cols = ["step"] + [f"c_a[{b + 1}][2]" for b in range(NA)]
    cols += [f"c_a[{past(b, NA)}][3]" for b in BINS_A] + [f"c_b[{past(b, NB)}][3]" for b in BINS_B]
    text = (HEADER.replace("FIX", "fix 1 all nve/mdp bricks yes") + f"compute a all rdf/mdp {NA}\ncompute b all rdf/mdp {NB}\n"
            "thermo_style custom " + " ".join(cols) + "\nrun 200\n")
    out = {}
    for np_ in (1, 2, 4):
        rc, so, err = _run(text, timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        assert "Loaded 1 plugins from rdfmdpplugin.so" in so
        m = re.search(r"fix nve/mdp: (\d+) bricks, (\d+) reneighborings on the device", so)
        assert int(m.group(1)) == np_ and int(m.group(2)) >= 20              # the remap ran many times: every atom left the box
        out[np_] = np.array(_thermo_rows(so))
    return out


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_a_drifting_crystal_reads_its_shells(drift_runs, np_):
    rows = drift_runs[np_]
    assert [int(s) for s in rows[:, 0]] == [0, 40, 80, 120, 160, 200] and rows.shape[1] == 1 + NA + 10
    want = np.array([c for _, c in SHELLS], dtype=float)
    for r in rows:
        g, coord = r[1:1 + NA], r[1 + NA:1 + NA + 5]
        assert np.all(np.abs(coord - want) <= 1e-6 * want), (r[0], coord)    # the mini-host prints 8 digits
        empty = [b for b in range(NA) if b not in BINS_A]
        assert np.all(g[empty] == 0.0) and np.all(g[BINS_A] > 1.0), (r[0], g)


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_two_computes_on_one_run_both_read_right(drift_runs, np_):
    """a context holds one measurement: each compute finds the other's setup in its place (mdp_rdf_info's serial) and sends
    its own again; the 44-bin compute reads the same shells as the 28-bin one at every row"""
    rows = drift_runs[np_]
    want = np.array([c for _, c in SHELLS], dtype=float)
    for r in rows:
        assert np.all(np.abs(r[1 + NA + 5:] - want) <= 1e-6 * want), (r[0], r[1 + NA + 5:])


HOT = """plugin load aeamplugin.so
plugin load rdfmdpplugin.so
units metal
lattice fcc 4.045
region MeSi block 0 6 0 6 0 6
region low block 0 6 0 6 0 3
create_box 2 MeSi
create_atoms 1 region MeSi
pair_style aeam
pair_coeff * * ../tests/golden/potentials/AlSi.aeam Al Si
neighbor 1.0 bin
neigh_modify every 1 delay 0 check yes
set region MeSi type/fraction 2 0.05 7683797
timestep 0.001
velocity all create 2500.0 1082337
group low region low
group al type 1
group si type 2
group lowal intersect low al
group lowsi intersect low si
fix 1 all nve/mdp bricks yes
compute r low rdf/mdp 25 1 1 1 2
thermo_style custom step c_r[11][2] c_r[12][2] c_r[20][2] c_r[25][3] c_r[11][4] c_r[12][4] c_r[20][4] c_r[25][5]
thermo 25
run 100
"""


def test_the_hot_alloy_reads_the_same_rows_on_1_and_2_ranks():
    """2 500 K, 5 % Si, the lower half of the box as the group (membership by tag, taken at the start of the run: atoms
    leave the region and stay members), the columns 1-1 and 1-2.  The trajectories of 1 and 2 bricks differ in the last
    bits, so a pair may sit on the other side of a bin edge: the rows agree to within 2 pair counts.  One pair count is
      1 / (vfrac_b normfac icount)  in a g column, vfrac_b = 4 pi / (3 V) ((b + 1)^3 - b^3) delr^3, and
      1 / icount                    in a coordination column,
    with icount = the Al atoms of the group for both columns, normfac = icount - 1 for 1-1 and = the group's Si atoms for
    1-2; on top of that the two prints of 8 digits."""
    rows, counts = {}, None
    for np_ in (1, 2):
        rc, out, err = _run(HOT, timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        rows[np_] = np.array(_thermo_rows(out))
        counts = {g: int(n) for n, g in re.findall(r"(\d+) atoms in group (\w+)", out)}
    n_al, n_si = counts["lowal"], counts["lowsi"]
    assert n_al + n_si == counts["low"] and n_si > 5 and 400 < counts["low"] < 520
    assert rows[1].shape == rows[2].shape == (5, 9)
    delr, const = CUTFORCE / 25, 4.0 * math.pi / (3.0 * (6 * A) ** 3)
    vfrac = lambda b: const * ((b + 1) ** 3 - b ** 3) * delr ** 3             # b: 0-based bin
    unit = np.array([1.0 / (vfrac(10) * (n_al - 1) * n_al), 1.0 / (vfrac(11) * (n_al - 1) * n_al), 1.0 / (vfrac(19) * (n_al - 1) * n_al),
                     1.0 / n_al,
                     1.0 / (vfrac(10) * n_si * n_al), 1.0 / (vfrac(11) * n_si * n_al), 1.0 / (vfrac(19) * n_si * n_al), 1.0 / n_al])
    a, b = rows[1][:, 1:], rows[2][:, 1:]
    assert np.all(np.abs(a - b) <= 2.0 * unit + 2e-7 * np.abs(a)), (a, b, unit)
    # not vacuous: the first shell (2.86 A, bins 11 and 12 of 0.26 A) is occupied in both columns, and an Al atom of the group
    # has most of a crystal's 78 neighbours within 6.5 A -- fewer than 78 x 0.95: partners outside the group do not count
    assert np.all(a[:, 0] + a[:, 1] > 1.0) and np.all(a[:, 4] + a[:, 5] > 0.5)
    assert np.all((a[:, 3] > 40.0) & (a[:, 3] < 74.0)) and np.all((a[:, 7] > 1.0) & (a[:, 7] < 6.0)), a


@pytest.mark.parametrize("fix,compute,msg", [
    ("fix 1 all nve/mdp", "compute r all rdf/mdp 28",
     "runs in the host-linked mode, where the host's atom->x and neighbour list are current: use compute rdf"),
    ("fix 1 all nve", "compute r all rdf/mdp 28", "Compute rdf/mdp requires fix nve/mdp"),
    ("fix 1 all nve/mdp bricks yes", "compute r all rdf/mdp 28 cutoff 6.6",
     "cutoff 6.6 is beyond the pair style's cutforce 6.5"),
])
def test_refusals_that_need_a_run(fix, compute, msg):
    rc, out, err = _run(HEADER.replace("FIX", fix) + compute + "\nthermo_style custom step c_r[1][2]\nrun 10\n", timeout=600)
    assert rc == 1
    assert msg in err, err


def test_the_examples_run():
    """examples/in.rebomos-bulk.rdf-mdp.mi355x: a Mo has 6 S within 2.8 A and 6 Mo within 3.5 A at every row (300 K: no bond
    breaks); examples/in.aeam-alsi.rdf-mdp.mi355x: the heated alloy keeps about 12 x 0.95 Al around an Al within 3.5 A"""
    rc, out, err = _run(script_file="examples/in.rebomos-bulk.rdf-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 25, 50, 75, 100]
    assert np.all(rows[:, 3] > 5.0) and np.all(rows[:, 4] == 6.0) and np.all(rows[:, 5] == 6.0) and np.all(rows[:, 6] > 150.0)
    rc, out, err = _run(script_file="examples/in.aeam-alsi.rdf-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 50, 100, 150, 200]
    assert np.all(np.abs(rows[:, 4] - 12 * 0.95) < 0.6) and np.all(rows[:, 5] < 2.0) and np.all(rows[:, 7] > 60.0)
