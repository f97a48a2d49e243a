"""GPU: `compute profile/mdp` through `plugin load` + `run` in the mini-host -- the drifting 0 K crystal of
tests/test_gpu_msd_mdp_plugin.py on 1, 2 and 4 ranks with two computes on one run; the hot alloy with a group on a region on
1 and 2 ranks; the refusals that need a run to be seen; and the example input."""
import re

import numpy as np
import pytest

from conftest import POT_AEAM
from lammps_plugins_amd.host import capi, system as S
from test_plugin_boundary import _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env
from test_gpu_msd_mdp_plugin import DRIFT

pytestmark = pytest.mark.gpu

HEADER = DRIFT.replace("plugin load msdmdpplugin.so", "plugin load profilemdpplugin.so")
VDRIFT = np.array([250.0, -125.0, 62.5])          # `velocity all set` of DRIFT
NATOMS = 864
NP_, NQ = 7, 12                                  # rows of p (x 7) and of q (x 3 z 4)


def _cols(cid, rows, ndim):
    """count, temp and the three vcm columns of every row"""
    return [f"c_{cid}[{b}][{ndim + k}]" for b in range(1, rows + 1) for k in (1, 4, 5, 6, 7)]


@pytest.fixture(scope="module")
def drift_runs():
    text = (HEADER.replace("FIX", "fix 1 all nve/mdp bricks yes") + "compute p all profile/mdp x 7 com yes\n"
            "compute q all profile/mdp x 3 z 4\nthermo_style custom step " + " ".join(_cols("p", NP_, 1) + _cols("q", NQ, 2))
            + "\nrun 200\n")
    out = {}
    for np_ in (1, 2, 4):
        rc, so, err = _run(text, timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        assert "Loaded 1 plugins from profilemdpplugin.so" in so
        m = re.search(r"fix nve/mdp: (\d+) bricks, (\d+) reneighborings on the device", so)
        assert int(m.group(1)) == np_ and int(m.group(2)) >= 20              # the remap ran many times: every atom left the box
        out[np_] = np.array(_thermo_rows(so))
    return out


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_a_drifting_crystal_reads_its_drift_in_every_bin(drift_runs, np_):
    """two computes on one run (each finds the other's bins in its place by mdp_profile_info's serial and sends its own
    again): at every thermo row the counts sum to natoms, every non-empty bin's vcm is the drift, the temperature about the
    bin's own flow (p, com yes) is zero and the one that counts the flow (q, com no) is m |v|^2 mvv2e / (3 boltz)"""
    rows = drift_runs[np_]
    assert [int(s) for s in rows[:, 0]] == [0, 40, 80, 120, 160, 200] and rows.shape[1] == 1 + 5 * (NP_ + NQ)
    mass = float(capi.AeamFile(POT_AEAM).mass[0])
    tflow = mass * float(VDRIFT @ VDRIFT) * S.MVV2E / (3.0 * S.BOLTZ)
    for r in rows:
        p, q = r[1:1 + 5 * NP_].reshape(NP_, 5), r[1 + 5 * NP_:].reshape(NQ, 5)
        for t, rows_ in ((p, NP_), (q, NQ)):
            assert t[:, 0].sum() == NATOMS and np.all(t[:, 0] == np.rint(t[:, 0])), (r[0], t[:, 0])
            full = t[:, 0] > 0
            assert full.sum() >= rows_ - 1
            assert np.all(np.abs(t[full, 2:] - VDRIFT) <= 1e-6 * np.abs(VDRIFT)), (r[0], t[:, 2:])
            assert np.all(t[~full, 1:] == 0.0)
        assert np.all(np.abs(p[:, 1]) <= 1e-6), (r[0], p[:, 1])
        fq = q[:, 0] > 0
        assert np.all(np.abs(q[fq, 1] - tflow) <= 1e-6 * tflow), (r[0], q[:, 1], tflow)


HOT = """plugin load aeamplugin.so
plugin load profilemdpplugin.so
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
fix 1 all nve/mdp bricks yes
compute g low profile/mdp z 7
compute a all profile/mdp z 7
thermo_style custom step temp COLS
thermo 25
run 100
"""


@pytest.mark.parametrize("np_", [1, 2])
def test_the_hot_alloy_by_region_and_against_thermo(np_):
    """2 500 K, 5 % Si, 7 bins along z.  The group is the lower half of the box (planes k / 12, k = 0 .. 6, of the box
    height; the bin edge 4 / 7 lies between the planes 6 and 7): at step 0 its bins 5 .. 7 are empty and the others hold all
    of it.  Over all atoms, sum_b count_b temp_b / N is the kinetic temperature with 3 N degrees of freedom: thermo's temp,
    which has 3 N - 3, times (3 N - 3) / 3 N."""
    cols = [f"c_g[{b}][2]" for b in range(1, 8)] + [f"c_a[{b}][{k}]" for b in range(1, 8) for k in (2, 5)]
    rc, out, err = _run(HOT.replace("COLS", " ".join(cols)), timeout=600, np=np_,
                        env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    nlow = {g: int(n) for n, g in re.findall(r"(\d+) atoms in group (\w+)", out)}["low"]
    assert rows.shape == (5, 2 + 7 + 14) and 400 < nlow < 520
    g0 = rows[0, 2:9]
    assert np.all(g0[4:] == 0.0) and g0[:4].sum() == nlow and np.all(g0[:4] > 0), g0
    for r in rows:
        a = r[9:].reshape(7, 2)
        assert r[2:9].sum() == nlow and a[:, 0].sum() == NATOMS              # membership goes with the atoms; nobody is lost
        tmean = (a[:, 0] * a[:, 1]).sum() / NATOMS
        want = r[1] * (3.0 * NATOMS - 3.0) / (3.0 * NATOMS)
        assert abs(tmean - want) <= 1e-6 * want and want > 500.0, (r[0], tmean, want)
    assert rows[-1, 1] < rows[0, 1]          # (the lattice takes half the kinetic energy)


@pytest.mark.parametrize("fix,msg", [
    ("fix 1 all nve/mdp", "runs in the host-linked mode, where the host's atom->x and atom->v are current: use compute chunk/atom"),
    ("fix 1 all nve", "Compute profile/mdp requires fix nve/mdp"),
])
def test_refusals_that_need_a_run(fix, msg):
    rc, out, err = _run(HEADER.replace("FIX", fix) + "compute p all profile/mdp x 7\nthermo_style custom step c_p[1][2]\nrun 10\n",
                        timeout=600)
    assert rc == 1
    assert msg in err, err


def test_the_example_runs():
    """examples/in.aeam-alsi.profile-mdp.mi355x: the strip is bin 1 of 8, 6 planes of 72 atoms at step 0.  The plane at x = 0
    sits on the edge between bins 8 and 1, and the hot strip expands: up to that whole plane may leave bin 1, no more.  The
    mass density follows the count (2.70 g/cm^3 for 432 atoms of Al with 0.75 % Si).  The strip goes to 900 K, the middle of
    the bar stays near the 50 K that 100 K of initial velocities leave a harmonic crystal, and the bins next to the strip
    are warmer than the middle at the end."""
    rc, out, err = _run(script_file="examples/in.aeam-alsi.profile-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 100, 200, 300, 400, 500] and rows.shape[1] == 10
    assert rows[0, 2] == 432 and np.all((rows[:, 2] >= 432 - 72) & (rows[:, 2] <= 432 + 72)), rows[:, 2]
    assert np.all(np.abs(rows[:, 9] / (2.70 * rows[:, 2] / 432.0) - 1.0) < 0.01), rows[:, 9]
    assert np.all(np.abs(rows[0, 3:9] - 100.0) < 25.0)
    assert 600.0 < rows[-1, 3] < 1200.0 and rows[-1, 6] < 150.0
    assert min(rows[-1, 4], rows[-1, 8]) > rows[-1, 6]
