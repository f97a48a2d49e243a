"""GPU: `compute adf/mdp` through `plugin load` + `run` in the mini-host -- the drifting perfect fcc crystal of
tests/test_gpu_msd_mdp_plugin.py, whose first shell holds 48, 24, 48 and 12 ordered angles of 60, 90, 120 and 180 degrees
per atom, on 1, 2 and 4 ranks; a second compute in the cosine on the same run; the hot alloy with a group on 1 and 2
ranks; the refusals that need a run to be seen; and the two examples."""
import re

import numpy as np
import pytest

from test_plugin_boundary import _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env
from test_gpu_msd_mdp_plugin import DRIFT

pytestmark = pytest.mark.gpu

HEADER = DRIFT.replace("plugin load msdmdpplugin.so", "plugin load adfmdpplugin.so")
NA, NB = 25, 25
ANGLES = [(60.0, 48), (90.0, 24), (120.0, 48), (180.0, 12)]            # degrees, ordered pairs per atom of the fcc first shell


def _bins():
    """0-based bins of the four angles in degrees and in the cosine, each at least a quarter of a bin from its edges (180
    degrees and cos = -1 sit at the closed ends of the range, where there is no edge): a 0 K lattice is read here, and no
    rounding of an angle may decide its bin.  An odd Nbin keeps cos 90 = 0 mid-bin, and -1/2 and 1/2 at a quarter."""
    deg = [u * NA / 180.0 for u, _ in ANGLES]
    cos = [(np.cos(np.radians(u)) + 1.0) * NB / 2.0 for u, _ in ANGLES]
    assert NB % 2 == 1 and all(0.25 - 1e-12 <= t % 1.0 <= 0.75 + 1e-12 for t in deg[:3] + cos[:3]), (deg, cos)
    assert abs(cos[1] % 1.0 - 0.5) < 1e-12 and abs(cos[0] % 1.0 - 0.75) < 1e-12 and abs(cos[2] % 1.0 - 0.25) < 1e-12
    return [min(int(t), NA - 1) for t in deg], [int(round(t - (t % 1.0))) for t in cos[:3]] + [0]


BINS_A, BINS_B = _bins()


@pytest.fixture(scope="module")
def drift_runs():
    """the crystal going twice through the box in 200 steps, with compute a (25 bins of degrees) and compute b (25 bins of the
    cosine) on the same run, on 1, 2 and 4 ranks: step, the first column of all 25 bins of a, then the angles per centre of
    a at the row just past each peak (the last peak sits in the last row: read there) and of b likewise, in the order of
    b's bins (180, 120, 90, 60 degrees)"""
    assert BINS_A == [8, 12, 16, 24] and BINS_B == [18, 12, 6, 0]
    cols = ["step"] + [f"c_a[{b + 1}][2]" for b in range(NA)]
    cols += [f"c_a[{min(b + 1, NA - 1) + 1}][3]" for b in BINS_A] + [f"c_b[{min(b + 1, NB - 1) + 1}][3]" for b in sorted(BINS_B)]
    text = (HEADER.replace("FIX", "fix 1 all nve/mdp bricks yes") + f"compute a all adf/mdp {NA} * * * 0 3.5 0 3.5 cumulative centre\n"
            f"compute b all adf/mdp {NB} * * * 0 3.5 0 3.5 ordinate cosine cumulative centre\n"
            "thermo_style custom " + " ".join(cols) + "\nrun 200\n")
    out = {}
    for np_ in (1, 2, 4):
        rc, so, err = _run(text, timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        assert "Loaded 1 plugins from adfmdpplugin.so" in so
        m = re.search(r"fix nve/mdp: (\d+) bricks, (\d+) reneighborings on the device", so)
        assert int(m.group(1)) == np_ and int(m.group(2)) >= 20              # the remap ran many times: every atom left the box
        out[np_] = np.array(_thermo_rows(so))
    return out


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_a_drifting_crystal_reads_its_angles(drift_runs, np_):
    """at every thermo row the first column is non-zero exactly in rows 9, 13, 17 and 25, and the angles per centre just past
    each peak are 48, 72, 120 and 132 -- whole numbers over a whole number, exact in the 8 printed digits"""
    rows = drift_runs[np_]
    assert [int(s) for s in rows[:, 0]] == [0, 40, 80, 120, 160, 200] and rows.shape[1] == 1 + NA + 8
    for r in rows:
        f, cum = r[1:1 + NA], r[1 + NA:1 + NA + 4]
        assert [b + 1 for b in range(NA) if f[b] != 0.0] == [9, 13, 17, 25], (r[0], f)
        assert cum.tolist() == [48.0, 72.0, 120.0, 132.0], (r[0], cum)
        # hist / (count delta), delta = 7.2 degrees, to the 8 printed digits
        assert np.allclose(f[BINS_A], np.array([48, 24, 48, 12]) / (132 * 7.2), rtol=2e-7, atol=0.0)


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_two_computes_on_one_run_both_read_right(drift_runs, np_):
    """a context holds one adf measurement: each compute finds the other's setup in its place (mdp_adf_info's serial) and
    sends its own again; in the cosine the peaks come in the order 180, 120, 90, 60 degrees: 12, 60, 84, 132 per centre"""
    for r in drift_runs[np_]:
        assert r[1 + NA + 4:].tolist() == [12.0, 60.0, 84.0, 132.0], (r[0], r[1 + NA + 4:])


HOT = """plugin load aeamplugin.so
plugin load adfmdpplugin.so
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
compute a low adf/mdp 25 1 1 1 0 3.5 0 3.5 1 1 2 0 3.5 0 3.5 cumulative centre
thermo_style custom step c_a[9][2] c_a[13][2] c_a[17][2] c_a[25][3] c_a[9][4] c_a[13][4] c_a[17][4] c_a[25][5]
thermo 25
run 100
"""


def test_the_hot_alloy_reads_the_same_rows_on_1_and_2_ranks():
    """2 500 K, 5 % Si, the lower half of the box as the group (membership by tag, taken at the start of the run), the
    triples Al-Al-Al and Al-Al-Si around the group's Al atoms.  The trajectories of 1 and 2 bricks differ in the last bits,
    so an angle may sit on the other side of a bin edge (in both orders where j and k are drawn alike): the rows agree to
    within 2 angle counts.  One angle count is
      1 / (count delta)   in a distribution column, count = the triple's angles = its last cumulative row x icount,
      1 / icount          in a cumulative column,
    with delta = 7.2 degrees and icount = the Al atoms of the group for both triples; on top of that the two prints of 8
    digits."""
    rows, counts = {}, None
    for np_ in (1, 2):
        rc, out, err = _run(HOT, timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        rows[np_] = np.array(_thermo_rows(out))
        counts = {g: int(n) for n, g in re.findall(r"(\d+) atoms in group (\w+)", out)}
    n_al, n_si = counts["lowal"], counts["lowsi"]
    assert n_al + n_si == counts["low"] and n_si > 5 and 400 < counts["low"] < 520
    assert rows[1].shape == rows[2].shape == (5, 9)
    a, b = rows[1][:, 1:], rows[2][:, 1:]
    unit = np.empty_like(a)
    for k, last in ((0, 3), (4, 7)):
        unit[:, k:k + 3] = 1.0 / (a[:, last:last + 1] * n_al * 7.2)
        unit[:, last] = 1.0 / n_al
    assert np.all(np.abs(a - b) <= 2.0 * unit + 2e-7 * np.abs(a)), (a, b, unit)
    # not vacuous: an Al of the group has most of a crystal's 12 first neighbours among the group's Al (fewer than 12 x 11
    # ordered pairs: partners outside the group do not count, and at 2 500 K some have left the shell), far fewer pairs
    # with a Si in them, and the crystal's peaks are still occupied at step 0
    assert np.all((a[:, 3] > 40.0) & (a[:, 3] < 132.0)) and np.all((a[:, 7] > 0.5) & (a[:, 7] < 0.2 * a[:, 3])), a
    assert np.all(a[0, :3] > 0.0) and np.all(a[0, 4:7] > 0.0)


@pytest.mark.parametrize("fix,compute,msg", [
    ("fix 1 all nve/mdp", "compute a all adf/mdp 25",
     "runs in the host-linked mode, where the host's atom->x and neighbour list are current: use compute adf"),
    ("fix 1 all nve", "compute a all adf/mdp 25", "Compute adf/mdp requires fix nve/mdp"),
    ("fix 1 all nve/mdp bricks yes", "compute a all adf/mdp 25 * * * 0 3.5 0 6.6",
     "the outer radius 6.6 of triple 1 is beyond the pair style's cutforce 6.5"),
])
def test_refusals_that_need_a_run(fix, compute, msg):
    rc, out, err = _run(HEADER.replace("FIX", fix) + compute + "\nthermo_style custom step c_a[1][2]\nrun 10\n", timeout=600)
    assert rc == 1
    assert msg in err, err


def test_the_default_triple_is_both_shells_up_to_cutforce():
    """no triple: * * * with both shells 0 .. cutforce = 6.5 A, the 78 neighbours of five fcc shells, under the cap of 128: the
    run reads 78 x 77 angles per atom in the last row"""
    rc, out, err = _run(HEADER.replace("FIX", "fix 1 all nve/mdp bricks yes") + "compute a all adf/mdp 25 cumulative centre\n"
                        "thermo_style custom step c_a[25][3]\nrun 40\n", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert rows[:, 1].tolist() == [78.0 * 77.0] * len(rows) and len(rows) == 2


def test_the_examples_run():
    """examples/in.rebomos-bulk.adf-mdp.mi355x: at every row a Mo has 30 ordered S-Mo-S angles, about 18 of them in the bin of 81
    - 82 degrees and the rest in that of 135, none near 180, and an S its 6 Mo-S-Mo angles, all in one bin of 18 degrees
    (300 K: no bond breaks, and hardly an angle strays 9 degrees);
    examples/in.aeam-alsi.adf-mdp.mi355x: the crystal's 132 angles per Al at step 0 with nothing between the peaks; once
    heated the 60-degree peak is lower, the bin between the peaks is filled, and an Al keeps between 9 and 14 neighbours
    within 3.5 A (n (n - 1) between 72 and 182: a hot dense metal neither opens up nor packs tighter than that)"""
    rc, out, err = _run(script_file="examples/in.rebomos-bulk.adf-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 25, 50, 75, 100]
    assert np.all(rows[:, 6] == 30.0) and np.all(rows[:, 8] == 6.0) and np.all(rows[:, 4] == 0.0)
    assert np.all(rows[:, 2] > 0.0) and np.all(rows[:, 3] > 0.0) and np.all(np.abs(rows[:, 5] - 18.0) < 1.5) and np.all(rows[:, 7] > 0.045)
    rc, out, err = _run(script_file="examples/in.aeam-alsi.adf-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 50, 100, 150, 200]
    assert rows.shape[1] == 8 and rows[0, 7] == 132.0 and rows[0, 5] == 0.0 and np.all(rows[0, [3, 4, 6]] > 0.0)
    assert np.all(rows[1:, 5] > 0.0) and np.all(rows[1:, 3] < rows[0, 3]) and np.all((rows[1:, 7] > 72.0) & (rows[1:, 7] < 182.0))
