"""GPU: `compute msd/mdp` through `plugin load` + `run` in the mini-host -- a rigid drift whose values are (v t)^2, the hot
alloy of examples/in.aeam-alsi.msd-mdp.mi355x on 1, 2 and 4 ranks, atom->image coming back from a bricks run as the
host-linked mode leaves it, and the refusals that need a run to be seen."""
import os
import re

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env

pytestmark = pytest.mark.gpu
ROW_REL = 2e-7     # two 8-digit prints of one value

# a perfect fcc crystal (no net force on any atom) of 6 x 6 x 6 cells, box 24.27 A, every atom at (250, -125, 62.5) A/ps:
# 50 A along x in 200 steps -- twice through the box --, 25 A against y, 12.5 A along z
V = (250.0, -125.0, 62.5)
DRIFT = """plugin load aeamplugin.so
plugin load msdmdpplugin.so
units metal
lattice fcc 4.045
region MeSi block 0 6 0 6 0 6
create_box 2 MeSi
create_atoms 1 region MeSi
pair_style aeam
pair_coeff * * ../tests/golden/potentials/AlSi.aeam Al Si
neighbor 2.0 bin
neigh_modify every 1 delay 0 check yes
timestep 0.001
velocity all set 250.0 -125.0 62.5
FIX
thermo 40
"""
MSD = """compute m all msd/mdp
compute c all msd/mdp com yes
thermo_style custom step c_m[1] c_m[2] c_m[3] c_m[4] c_c[4]
"""


def test_a_rigid_drift_reads_v_t_squared():
    rc, out, err = _run(DRIFT.replace("FIX", "fix 1 all nve/mdp bricks yes") + MSD + "run 200\n", timeout=600,
                        env=dict(MDP_FIX_STATS="1"))
    assert rc == 0, err[-3000:]
    assert "Loaded 1 plugins from msdmdpplugin.so" in out
    m = re.search(r"fix nve/mdp: 1 bricks, (\d+) reneighborings on the device", out)
    assert int(m.group(1)) >= 20                                # the remap ran many times: every atom left the box
    rows = _thermo_rows(out)
    assert [int(r[0]) for r in rows] == [0, 40, 80, 120, 160, 200]
    assert 200 * 0.001 * V[0] > 2 * 6 * 4.045                   # twice through the box
    for r in rows:
        t = r[0] * 0.001
        want = [(v * t) ** 2 for v in V]
        want.append(sum(want))
        for got, w in zip(r[1:5], want):
            assert abs(got - w) <= 1e-6 * w, (r, want)          # the mini-host prints 8 digits
        assert abs(r[5]) < 1e-12                                # com yes: a rigid drift is all centre of mass


def _images(path):
    rows = np.array([[float(v) for v in l.split()] for l in path.read_text().splitlines()[5:]])
    return rows[:, 0].astype(int), rows[:, 1:4], rows[:, 7:10].astype(int)


@pytest.mark.parametrize("case", ["drift", "hot"])
def test_the_host_gets_the_image_flags_a_hostlinked_run_leaves(case, tmp_path):
    """atom->image after a bricks run (the device's remap counted the box vectors) against the same run in the host-linked
    mode (the host's own remap did); a `run 0` behind each brings every atom into the box, so that the two hosts hold
    the same wrapped coordinates and the flags can be compared one by one"""
    head = DRIFT if case == "drift" else DRIFT.replace("velocity all set 250.0 -125.0 62.5", "velocity all create 2500.0 1082337").replace(
        "neighbor 2.0 bin", "neighbor 1.0 bin")
    got = {}
    for mode, fix in (("host", "fix 1 all nve/mdp"), ("bricks", "fix 1 all nve/mdp bricks yes")):
        dump = tmp_path / f"{case}.{mode}"
        rc, out, err = _run(head.replace("FIX", fix) + f"run 200\nrun 0\nwrite_dump all custom {dump} id x y z vx vy vz ix iy iz\n",
                            timeout=600)
        assert rc == 0, err[-3000:]
        got[mode] = _images(dump)
    (ida, xa, ia), (idb, xb, ib) = got["host"], got["bricks"]
    assert len(ida) == 864 and np.array_equal(ida, idb)
    assert np.abs(xa - xb).max() < 1e-8                         # the same trajectory (the bound of the dd net's positions)
    assert np.array_equal(ia, ib)
    if case == "drift":
        assert np.all(ia[:, 0] >= 2) and np.all(ia[:, 1] <= -1) and ia[:, 2].max() == 1
    else:
        assert 10 < np.any(ia != 0, axis=1).sum() < 864         # some atoms diffused through a face at 2 500 K, not all


@pytest.fixture(scope="module")
def example_text():
    text = open(os.path.join(PKG, "examples", "in.aeam-alsi.msd-mdp.mi355x")).read()
    for want in ("region MeSi block 0 20 0 20 0 20", "fix 1 all nvt/mdp temp 863.0 863.0 0.1 bricks yes", "compute m all msd/mdp",
                 "thermo_style custom step temp etotal pe c_m[1] c_m[2] c_m[3] c_m[4]", "thermo 100", "run 1000"):
        assert want in text
    # the example's alloy at 8 x 8 x 8 cells (2 048 atoms), 200 steps, a row every 50
    return text.replace("block 0 20 0 20 0 20", "block 0 8 0 8 0 8").replace("thermo 100", "thermo 50").replace("run 1000", "run 200")


def test_the_example_runs_under_the_thermostat(example_text):
    rc, out, err = _run(example_text, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 50, 100, 150, 200]
    assert not rows[0, 4:8].any()
    assert np.all(rows[1:, 7] > 0.01) and np.all(rows[1:, 7] < 5.0)          # thermal motion at 863 K: tenths of an A^2
    assert np.allclose(rows[:, 4] + rows[:, 5] + rows[:, 6], rows[:, 7], rtol=1e-6)


def test_the_hot_alloy_reads_the_same_msd_on_1_2_and_4_ranks(example_text):
    """fix nvt/mdp is a one-rank thermostat, so the ranks are compared under `fix nve/mdp bricks yes` from the example's
    863 K velocities: the MSD rows of 2 and 4 bricks (atoms migrate, their origins are found by tag on the new rank) are
    the one-brick rows to the printed digits"""
    text = example_text.replace("fix 1 all nvt/mdp temp 863.0 863.0 0.1 bricks yes", "fix 1 all nve/mdp bricks yes")
    rows = {}
    for np_ in (1, 2, 4):
        rc, out, err = _run(text, timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        m = re.search(r"fix nve/mdp: (\d+) bricks, (\d+) reneighborings on the device", out)
        assert int(m.group(1)) == np_ and int(m.group(2)) >= 1
        rows[np_] = np.array(_thermo_rows(out))
    assert rows[1].shape == (5, 8) and rows[1][-1, 7] > 0.01
    for np_ in (2, 4):
        assert rows[np_].shape == rows[1].shape
        assert np.allclose(rows[np_][:, 4:8], rows[1][:, 4:8], rtol=ROW_REL, atol=0.0), (np_, rows[np_][:, 4:8], rows[1][:, 4:8])


@pytest.mark.parametrize("fix,msg", [
    ("fix 1 all nve/mdp", "runs in the host-linked mode, where the host keeps atom->image itself: use compute msd"),
    ("fix 1 all nve", "Compute msd/mdp requires fix nve/mdp"),
])
def test_refusals_that_need_a_run(fix, msg):
    rc, out, err = _run(DRIFT.replace("FIX", fix) + MSD + "run 10\n", timeout=600)
    assert rc == 1
    assert msg in err, err
