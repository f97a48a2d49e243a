"""GPU: `fix nvt/mdp` through `plugin load` + `run` in the mini-host -- sample.in's alloy with its own thermostat line
(examples/in.aeam-alsi.nvt-mdp.mi355x) and a REBO-MoS NVT input: the default (host-linked) mode against `bricks yes`,
the conserved quantity, two runs against one, the temperature the chain drives the alloy to, and the refusal of
several ranks.  The mini-host prints 8 significant digits (LAMMPS' "{:<14.8g}"): rows of the two modes are compared to
that precision."""
import os

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows

pytestmark = pytest.mark.gpu
ROW_REL = 2e-7     # two 8-digit prints of one value


def _script(path, **subs):
    text = open(os.path.join(PKG, "examples", path)).read()
    for old, new in subs.items():
        assert old in text, old
        text = text.replace(old, new)
    return text


AEAM = "in.aeam-alsi.nvt-mdp.mi355x"
FIX = "fix 1 all nvt/mdp temp 863.0 863.0 0.1\n"


def _rows(script, np_=1):
    rc, out, err = _run(script, timeout=900, np=np_)
    assert rc == 0, err[-3000:]
    assert "Loaded 1 plugins from nvtmdpplugin.so" in out
    return np.array(_thermo_rows(out))


def _rows_nve(script):
    rc, out, err = _run(script, timeout=900)
    assert rc == 0, err[-3000:]
    return np.array(_thermo_rows(out))


def _agree(a, b, cols):
    assert a.shape == b.shape
    for c in cols:
        assert np.allclose(a[:, c], b[:, c], rtol=ROW_REL, atol=1e-9), (c, a[:, c], b[:, c])


def test_aeam_example_both_modes_agree_and_conserve():
    """step temp etotal pe f_1 econserve press: 200 steps, thermo 20, host-linked against `bricks yes`"""
    base = dict([("run 1000", "run 200"), ("thermo 100", "thermo 20")])
    a = _rows(_script(AEAM, **base))
    b = _rows(_script(AEAM, **base, **{FIX: FIX.replace("0.1\n", "0.1 bricks yes\n")}))
    assert len(a) == 11
    _agree(a, b, (1, 3, 4))
    natoms = 32000
    # the NVE run of the same system, sampled alike: velocity Verlet's own fluctuation of the total energy at 1 fs
    nve = _rows_nve(_script("in.aeam-alsi.nve-mdp.mi355x", **dict([("run 400", "run 200"), ("thermo 100", "thermo 20")])))
    nve_spread = nve[:, 2].max() - nve[:, 2].min()
    for r in (a, b):
        assert abs(r[-1, 5] - r[0, 5]) / natoms < 2e-5                  # econserve = etotal + ecouple: no drift
        assert r[:, 5].max() - r[:, 5].min() < 1.5 * nve_spread + 0.02   # ... and it fluctuates as NVE's etotal does
        assert np.abs(r[:, 4]).max() > 1.0                                # the chain does exchange energy
        assert np.allclose(r[:, 5], r[:, 2] + r[:, 4], rtol=1e-7, atol=1e-3)


def test_two_runs_continue_the_chain_like_one():
    base = dict([("run 1000", "run 200"), ("thermo 100", "thermo 100")])
    one = _rows(_script(AEAM, **base))
    two = _rows(_script(AEAM, **dict([("run 1000", "run 100\nrun 100"), ("thermo 100", "thermo 100")])))
    assert one[-1][0] == two[-1][0] == 200
    for c in (1, 3, 4, 5):
        assert two[-1][c] == pytest.approx(one[-1][c], rel=ROW_REL, abs=1e-9), c


def test_rebomos_nvt_both_modes_agree():
    subs = {"plugin load rebomosplugin.so\n": "plugin load rebomosplugin.so\nplugin load nvtmdpplugin.so\n",
            "thermo_style custom step temp press pe ke cellgamma vol": "thermo_style custom step temp pe ke f_nvt econserve",
            "fix integrate all nve/mdp\nrun 20": "velocity all create 600.0 4928459\nfix nvt all nvt/mdp temp 300.0 300.0 0.05\nrun 200"}
    a = _rows(_script("in.rebomos-bulk.nve-mdp.mi355x", **subs))
    subs2 = dict(subs)
    subs2["fix integrate all nve/mdp\nrun 20"] = subs2["fix integrate all nve/mdp\nrun 20"].replace("0.05\n", "0.05 bricks yes\n")
    b = _rows(_script("in.rebomos-bulk.nve-mdp.mi355x", **subs2))
    _agree(a, b, (1, 2, 4))
    assert a[-1][1] < 550.0                                                # the chain pulls 600 K towards 300 K


def test_alloy_reaches_the_target_temperature():
    """32 000 atoms from 300 K with target 863 K: the mean temperature of the last 1 000 of 3 000 steps is within 2 %"""
    r = _rows(_script(AEAM, **dict([("run 1000", "run 3000"), ("thermo 100", "thermo 10"),
                                    ("velocity all create 863.0 1082337", "velocity all create 300.0 1082337")])))
    last = r[r[:, 0] > 2000]
    assert len(last) == 100
    assert abs(last[:, 1].mean() - 863.0) < 0.02 * 863.0


def test_several_ranks_are_refused():
    rc, out, err = _run(_script(AEAM, **{"run 1000": "run 10"}), np=2, timeout=300)
    assert rc == 1
    assert "one MPI rank only" in err
