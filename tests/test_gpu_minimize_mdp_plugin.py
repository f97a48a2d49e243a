"""GPU: `minimize/mdp` through `plugin load` in the mini-host, on the two example inputs cut to test size: the stats
block, the step counter and the time step afterwards, a following `fix nve/mdp` run that starts from the relaxed atoms,
thermo rows, and the same minimisation through host.resident.DeviceDomain.minimize."""
import os
import re

import numpy as np
import pytest

from conftest import POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from test_plugin_boundary import PKG, _run, _thermo_rows

pytestmark = pytest.mark.gpu
QUENCH = "in.rebomos-bulk.quench-mdp.mi355x"
ALLOY = "in.aeam-alsi.minimize-mdp.mi355x"
MIN = "minimize/mdp 0.0 1.0e-6 2000 20000\n"


def _script(path, **subs):
    text = open(os.path.join(PKG, "examples", path)).read()
    for old, new in subs.items():
        assert old in text, old
        text = text.replace(old, new)
    return text


def _stats(out):
    """the numbers of the `Minimization stats:` block"""
    m = re.search(r"Minimization stats:\n  Stopping criterion = (.+)\n  Energy initial, next-to-last, final = \n\s+(\S+)\s+(\S+)\s+(\S+)\n"
                  r"  Force two-norm initial, final = (\S+) (\S+)\n  Iterations, force evaluations = (\d+) (\d+)\n", out)
    assert m, out[-3000:]
    return dict(criterion=m.group(1), e_initial=float(m.group(2)), e_previous=float(m.group(3)), e_final=float(m.group(4)),
                fnorm_initial=float(m.group(5)), fnorm=float(m.group(6)), iterations=int(m.group(7)), evaluations=int(m.group(8)))


def _min_rows(out):
    """the minimiser's own rows (Step PotEng Fnorm)"""
    rows, grab = [], False
    for line in out.splitlines():
        if line.split() == ["Step", "PotEng", "Fnorm"]:
            grab = True
            continue
        if grab:
            p = line.split()
            if len(p) != 3 or not re.fullmatch(r"\d+", p[0]):
                grab = False
                continue
            rows.append([float(v) for v in p])
    return rows


def _md_rows(out, ncol):
    return [r for r in _thermo_rows(out) if len(r) == ncol]


def test_quench_of_the_hot_mos2_cell():
    """the example at 2 x 2 x 1 (1152 atoms), 100 MD steps from 300 K, the quench, then 20 NVE steps from the relaxed
    atoms with a time step the minimiser must have left alone"""
    text = _script(QUENCH, **{"replicate 4 4 2": "replicate 2 2 1", "run 200": "run 100",
                              MIN: MIN + "fix integrate all nve/mdp\nrun 20\n"})
    rc, out, err = _run(text, timeout=900)
    assert rc == 0, err[-3000:]
    assert "Loaded 1 plugins from minimizemdpplugin.so" in out
    st = _stats(out)
    assert st["criterion"] == "force tolerance" and st["fnorm"] < 1e-6 < st["fnorm_initial"]
    assert st["e_final"] < st["e_initial"] and 0 < st["iterations"] <= 2000 and st["evaluations"] == st["iterations"]
    rows = _md_rows(out, 5)                         # step temp press pe ke
    first = [r for r in rows if r[0] <= 100]
    second = [r for r in rows if r[0] > 100]
    assert first[-1][0] == 100
    # Step advanced by the iterations; row 0 of the second run is the relaxed structure, at rest up to the last iteration
    assert second[0][0] == 100 + st["iterations"] and second[-1][0] == 120 + st["iterations"]
    assert second[0][3] == pytest.approx(st["e_final"], rel=2e-8)
    assert second[0][1] < 1e-6                      # the velocities FIRE left (K)
    mrows = _min_rows(out)                          # `thermo 50`: the initial state, every 50 iterations, the last
    assert mrows[0][0] == 100 and mrows[0][1] == pytest.approx(st["e_initial"], rel=1e-11)
    assert [r[0] for r in mrows[1:-1]] == [100 + 50 * k for k in range(1, len(mrows) - 1)]
    assert mrows[-1][0] == 100 + st["iterations"] and mrows[-1][2] == pytest.approx(st["fnorm"], rel=1e-7)
    assert mrows[-1][1] < mrows[0][1] and mrows[-1][1] == pytest.approx(st["e_final"], rel=1e-11)
    m = re.search(r"Performance: \S+ ns/day, \S+ hours/ns, (\S+) timesteps/s", out[out.index("Minimization stats"):])
    assert m                                         # (the run's own line: 20 steps at 1 fs)


def test_alloy_is_relaxed_before_it_is_heated():
    """the example at 8 x 8 x 8 (2048 atoms, ~15 Si): minimise, then 200 thermostatted steps"""
    text = _script(ALLOY, **{"block 0 20 0 20 0 20": "block 0 8 0 8 0 8", "run 2000": "run 200", "thermo 100": "thermo 0"})
    rc, out, err = _run(text, timeout=900)
    assert rc == 0, err[-3000:]
    st = _stats(out)
    assert st["criterion"] == "force tolerance" and st["fnorm"] < 1e-6 < st["fnorm_initial"]
    assert st["e_final"] < st["e_initial"]
    assert _min_rows(out) == []                     # no thermo, no rows (and no blocking read per chunk)
    rows = _md_rows(out, 5)                         # step temp etotal pe press
    assert rows[0][0] == st["iterations"] and rows[-1][0] == st["iterations"] + 200
    assert rows[0][3] == pytest.approx(st["e_final"], rel=2e-8)
    assert rows[0][1] == pytest.approx(300.0, rel=1e-6)     # `velocity all create` after the minimisation


def _python_minimize(*args):
    ctx = capi.Context(0)
    try:
        p = capi.read_rebomos_file(POT_REBOMOS)
        ctx.rebomos_set_params(p)
        d = resident.DeviceDomain(ctx, capi.STYLE_REBOMOS, S.rebomos_bulk_cell(), 3.0 * p.rcmax[0][0] + 2.0, 2.0, [0, 0, 1], dt=0.001)
        return d.minimize(*args)
    finally:
        ctx.close()


def test_the_command_and_the_python_driver_agree():
    """The unrelaxed reference cell (288 atoms) through minimize/mdp and through DeviceDomain.minimize: the same library
    calls underneath.  The two hosts build the cell with their own arithmetic, so the coordinates agree to an ulp or
    so, not to the bit -- and this cell is a perfect crystal, whose in-plane forces are rounding noise that FIRE
    amplifies.  So the printed numbers are compared where that has not happened yet, after 100 iterations (maxiter), and
    at convergence the energies to the printed digits but not the count (971 and 973 iterations measured)."""
    base = _script(QUENCH, **{"replicate 4 4 2\n": "", "velocity all create 300.0 4928459\nfix integrate all nve/mdp\nrun 200\nunfix integrate\n": "",
                              "thermo 50": "thermo 0"})     # (no rows: a state read's energy compute gives the lists another history)
    rc, out, err = _run(base.replace(MIN, "minimize/mdp 0.0 0.0 100 20000\n"), timeout=900)
    assert rc == 0, err[-3000:]
    st, py = _stats(out), _python_minimize(0.0, 0.0, 100, 20000)
    print(f"minimize/mdp: {st}\nDeviceDomain.minimize: {py}")
    assert st["criterion"] == py["criterion"] == "max iterations"
    assert st["iterations"] == py["iterations"] == 100 and st["evaluations"] == py["evaluations"] == 100
    for k in ("e_initial", "e_final"):
        assert st[k] == pytest.approx(py[k], rel=1e-11), k          # %.12g
    for k in ("fnorm_initial", "fnorm"):
        assert st[k] == pytest.approx(py[k], rel=1e-7), k           # %.8g
    rc, out, err = _run(base, timeout=900)
    assert rc == 0, err[-3000:]
    st, py = _stats(out), _python_minimize(0.0, 1.0e-6, 2000, 20000)
    print(f"minimize/mdp: {st}\nDeviceDomain.minimize: {py}")
    assert st["criterion"] == py["criterion"] == "force tolerance"
    assert st["e_initial"] == pytest.approx(py["e_initial"], rel=1e-11)
    assert st["e_final"] == pytest.approx(py["e_final"], rel=1e-11)
    assert st["fnorm"] < 1e-6 and py["fnorm"] < 1e-6
    assert abs(st["iterations"] - py["iterations"]) <= 0.1 * py["iterations"]


def test_refusals_with_a_pair_style_loaded():
    base = _script(QUENCH, **{"replicate 4 4 2\n": "", "velocity all create 300.0 4928459\nfix integrate all nve/mdp\nrun 200\nunfix integrate\n": ""})
    rc, out, err = _run(base.replace("units metal", "units metal\nboundary p p f"), timeout=300)
    assert rc == 1 and "minimize/mdp needs a periodic box" in err, err[-2000:]
    rc, out, err = _run(base, timeout=300, np=2)
    assert rc == 1 and "minimize/mdp runs on one MPI rank" in err, err[-2000:]
    rc, out, err = _run(base, timeout=300, env={"MDP_REBOMOS_HOST_LIST": "1"})
    assert rc == 1 and "MDP_REBOMOS_HOST_LIST=1" in err, err[-2000:]
    rc, out, err = _run(base.replace(MIN, "timestep 0.0\n" + MIN), timeout=300)
    assert rc == 1 and "timestep must be > 0.0" in err, err[-2000:]
