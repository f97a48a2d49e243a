"""GPU: `fix langevin/mdp` through `plugin load` + `run` in the mini-host, handing its thermostat to `fix nve/mdp`:
the default (host-linked) mode against `bricks yes`, bricks of 2 and 4 ranks against one rank (the noise is keyed by
tag and step, so the trajectory does not depend on the rank count), the 32 000-atom alloy heated to 863 K, a REBO-MoS
cell held at 300 K with `tally yes` (econserve), the two fixes defined in either order, `unfix` between runs, and the
refusals that need a run (no fix nve/mdp, fix nvt/mdp, zero / tally on two ranks)."""
import os
import re

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env

pytestmark = pytest.mark.gpu
ROW_REL = 2e-7     # two 8-digit prints of one value
AEAM = "in.aeam-alsi.langevin-mdp.mi355x"
NVE = "fix integrate all nve/mdp\n"
LGV = "fix heat all langevin/mdp 300.0 863.0 0.1 48271\n"


def _script(path, **subs):
    text = open(os.path.join(PKG, "examples", path)).read()
    for old, new in subs.items():
        assert old in text, old
        text = text.replace(old, new)
    return text


def _rows(script, np_=1, env=None):
    rc, out, err = _run(script, timeout=900, np=np_, env=env)
    assert rc == 0, err[-3000:]
    assert "Loaded 1 plugins from langevinmdpplugin.so" in out
    return np.array(_thermo_rows(out)), out


def _short(**extra):
    return _script(AEAM, **dict([("run 2000", "run 200"), ("thermo 100", "thermo 20")]), **extra)


def test_default_mode_agrees_with_bricks_yes():
    a, _ = _rows(_short())
    b, _ = _rows(_short(**{NVE: "fix integrate all nve/mdp bricks yes\n"}))
    assert len(a) == 11 and a.shape == b.shape
    for c in (1, 2, 3):                                   # temp etotal pe
        assert np.allclose(a[:, c], b[:, c], rtol=ROW_REL, atol=1e-9), (c, a[:, c], b[:, c])
    assert a[-1, 1] > 400.0                               # the thermostat heats (the NVE run would cool towards 150 K)


@pytest.mark.parametrize("np_", [2, 4])
def test_bricks_of_several_ranks_follow_the_one_rank_run(np_):
    """the same trajectory on 1, 2 and 4 ranks: the thermostat needs no communication"""
    one, _ = _rows(_short(**{NVE: "fix integrate all nve/mdp bricks yes\n"}))
    many, out = _rows(_short(), np_=np_, env=_double_env())
    assert re.search(r"fix nve/mdp: %d bricks" % np_, out)
    assert one.shape == many.shape
    for a, b in zip(many, one):
        assert a[0] == b[0]
        for u, v in zip(a[1:], b[1:]):
            assert u == pytest.approx(v, rel=2e-8, abs=1e-6)


def test_alloy_is_heated_to_the_target():
    """the example's ramp 300 -> 863 K over 2000 steps (the temperature trails the ramp by the coupling time), then
    1000 steps held at 863 K by a second thermostat"""
    rows, _ = _rows(_script(AEAM, **{"run 2000": "run 2000\nunfix heat\nfix hold all langevin/mdp 863.0 863.0 0.1 48272\nrun 1000"}))
    assert rows[-1, 0] == 3000
    assert rows[20, 1] > 700.0                            # the end of the ramp
    assert np.mean(rows[-5:, 1]) == pytest.approx(863.0, rel=0.03)


def test_rebomos_cell_is_held_at_300k_and_econserve_stays_flat():
    """step temp press pe ke f_lgv econserve: the 3.98 M-atom cell from 300 K, 1000 steps (equipartition first takes
    half the kinetic energy into the lattice; the thermostat gives it back within a few coupling times)"""
    rows, _ = _rows(_script("in.rebomos-4m.langevin-mdp.mi355x", **{"run 100": "run 1000", "thermo 50": "thermo 100"}))
    assert rows[-1, 0] == 1000
    assert np.all(np.abs(rows[6:, 1] - 300.0) < 9.0)
    etotal = rows[:, 3] + rows[:, 4]
    drift_e, drift_c = abs(etotal[-1] - etotal[0]), abs(rows[-1, 6] - rows[0, 6])
    assert abs(rows[-1, 5]) > 10.0                        # the thermostat exchanged energy (eV)
    assert drift_c < 0.02 * drift_e


def test_fix_order_does_not_matter():
    a, _ = _rows(_short())
    b, _ = _rows(_short(**{NVE + LGV: LGV + NVE}))
    assert np.array_equal(a, b)


def test_unfix_between_runs_gives_nve():
    """run 100 with the thermostat, unfix it, run 100: the second run conserves etotal as NVE does"""
    text = _short(**{"run 200": "run 100\nunfix heat\nrun 100"})
    rows, out = _rows(text)
    first, second = rows[:6], rows[6:]
    assert abs(first[-1, 2] - first[0, 2]) > 50.0          # etotal moved under the thermostat
    assert np.ptp(second[:, 2]) < 0.5                      # ... and stays put without it (32 000 atoms)


@pytest.mark.parametrize("edit,msg", [
    ({NVE: ""}, "requires fix nve/mdp"),
    ({NVE: "fix integrate all nve\n"}, "requires fix nve/mdp"),
])
def test_refusals_at_run(edit, msg):
    rc, out, err = _run(_short(**edit), timeout=300)
    assert rc == 1 and msg in err, err[-2000:]


def test_nvt_mdp_is_a_second_thermostat():
    text = _short(**{"plugin load langevinmdpplugin.so\n": "plugin load langevinmdpplugin.so\nplugin load nvtmdpplugin.so\n",
                     NVE: "fix integrate all nvt/mdp temp 300.0 300.0 0.1\n"})
    rc, out, err = _run(text, timeout=300)
    assert rc == 1 and "use one thermostat" in err, err[-2000:]


@pytest.mark.parametrize("kw", ["zero yes", "tally yes"])
def test_zero_and_tally_refuse_two_ranks(kw):
    rc, out, err = _run(_short(**{LGV: LGV.replace("48271", "48271 " + kw)}), np=2, env=_double_env(), timeout=300)
    assert rc == 1 and "run on one MPI rank only" in err, err[-2000:]
