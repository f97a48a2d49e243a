"""GPU: `fix heat/mdp` through `plugin load` + `run` in the mini-host, handing its sources to one `fix nve/mdp` (its
Fix::extract("mdp_heat_sources") block).  The shipped ribbon example cut to 200 steps and an alloy deck written here, each
in the default (host-linked) mode and with `bricks yes`: the two modes agree on the thermo columns within what
tests/test_gpu_langevin_baths_plugin.py allows between them, f_hot > 1 > f_cold after step 1, the energy a source alone
puts in is F dt n and source and sink together leave etotal alone -- both to twice the largest excursion the same deck
shows under plain NVE, measured in the same test (the heated strip's integrator fluctuation grows with its temperature,
which rises by less than 20 % here).  Then the equilibrate-then-drive sequence (fix langevin/mdp, unfix, fix heat/mdp) and
the refusals of init() that need a run."""
import os
import re

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows

pytestmark = pytest.mark.gpu
ROW_REL = 2e-7     # two 8-digit prints of one value
F = 5.0            # eV/ps, the example's
DT = 0.001

ALLOY = """plugin load aeamplugin.so
plugin load heatmdpplugin.so
plugin load langevinmdpplugin.so
plugin load nvtmdpplugin.so
units metal
lattice fcc 4.045
region MeSi block 0 10 0 10 0 10
create_box 2 MeSi
create_atoms 1 region MeSi
pair_style aeam
pair_coeff * * ../tests/golden/potentials/AlSi.aeam Al Si
neighbor 1.0 bin
neigh_modify every 1 delay 0 check yes
set region MeSi type/fraction 2 0.0075 7683797
region floor block 0 10 0 10 0 2.9
region lowband block 0 10 1.0 4.0 0 10
region highband block 0 10 6.0 9.0 0 10
group substrate region floor
group mobile subtract all substrate
group inlow region lowband
group inhigh region highband
group hot intersect inlow mobile
group cold intersect inhigh mobile
timestep 0.001
velocity all create 300.0 1082337
velocity substrate set 0.0 0.0 0.0
fix integrate mobile nve/mdp
thermo_style custom step temp pe ke etotal f_hot f_cold
thermo 50
"""
HOT = f"fix hot hot heat/mdp 1 {F}\n"
COLD = f"fix cold cold heat/mdp 1 -{F}\n"
RUN = "run 200\n"


def _example():
    """the shipped example with `run 200` / `thermo 50` and the columns of the alloy deck"""
    text = open(os.path.join(PKG, "examples", "in.rebomos-ribbon.heat-mdp.mi355x")).read()
    assert f"fix hot  hot  heat/mdp 1  {F}" in text and f"fix cold cold heat/mdp 1 -{F}" in text
    text = re.sub(r"^thermo_style .*$", "thermo_style custom step temp pe ke etotal f_hot f_cold", text, flags=re.M)
    text = re.sub(r"^compute t .*\n", "", text, flags=re.M)
    text = text.replace("plugin load profilemdpplugin.so\n", "plugin load langevinmdpplugin.so\nplugin load nvtmdpplugin.so\n")
    text = text.replace("thermo 100\n", "thermo 50\n").replace("run 1000\n", "")
    assert "bricks yes" in text and "run" not in text.split("thermo 50")[1]
    hot = re.search(r"^fix hot .*\n", text, flags=re.M).group(0)
    cold = re.search(r"^fix cold .*\n", text, flags=re.M).group(0)
    return text.replace(hot, "").replace(cold, ""), hot, cold


def _deck(name, bricks):
    """(head without sources, hot, cold) of the ribbon (shipped with bricks yes) or the alloy (host-linked as written)"""
    if name == "ribbon":
        head, hot, cold = _example()
        return (head if bricks else head.replace(" bricks yes", "")), hot, cold
    return (ALLOY.replace("nve/mdp\n", "nve/mdp bricks yes\n") if bricks else ALLOY), HOT, COLD


def _rows(script, nrows=5, last=200):
    rc, out, err = _run(script, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert len(rows) == nrows and rows[-1, 0] == last, rows
    return rows


def _plain(head):
    """the deck without the fixes: f_hot / f_cold have nothing to print"""
    return head.replace(" f_hot f_cold", "")


_ROWS = {}


def _both(name, bricks):
    key = (name, bricks)
    if key not in _ROWS:
        head, hot, cold = _deck(name, bricks)
        _ROWS[key] = _rows(head + hot + cold + RUN)
    return _ROWS[key]


@pytest.mark.parametrize("name", ["ribbon", "alloy"])
def test_default_mode_agrees_with_bricks_yes_and_the_scales_straddle_one(name):
    a, b = _both(name, False), _both(name, True)
    assert a.shape == b.shape
    for c in (1, 2, 3, 4):                                              # temp pe ke etotal
        assert np.allclose(a[:, c], b[:, c], rtol=ROW_REL, atol=1e-9), (c, a[:, c], b[:, c])
    for c in (5, 6):                                                    # the scales: sums in another atom order
        assert np.allclose(a[:, c], b[:, c], rtol=ROW_REL, atol=1e-6), (c, a[:, c], b[:, c])
    for r in (a, b):
        assert r[0, 5] == 1.0 and r[0, 6] == 1.0                        # step 0 is not heated
        assert np.all(r[1:, 5] > 1.0) and np.all(r[1:, 6] < 1.0), (r[:, 5], r[:, 6])


@pytest.mark.parametrize("name,bricks", [("ribbon", True), ("alloy", False)])
def test_the_energy_put_in_is_the_flux_times_the_time(name, bricks, capsys):
    head, hot, cold = _deck(name, bricks)
    nve = _rows(_plain(head) + RUN)
    bound = 2.0 * float(np.abs(nve[:, 4] - nve[0, 4]).max())
    src = _rows(head.replace(" f_cold", "") + hot + RUN)
    n = src[:, 0]
    gained = src[:, 4] - src[0, 4]
    off = float(np.abs(gained - F * DT * n).max())
    both = _both(name, bricks)
    kept = float(np.abs(both[:, 4] - both[0, 4]).max())
    with capsys.disabled():
        print(f"heat/mdp {name}: source alone gained {gained[-1]:.6f} eV of {F * DT * n[-1]:.6f}, worst |dE - F dt n| {off:.3e} eV; source "
              f"and sink moved etotal by {kept:.3e} eV; bound 2 max|dE_nve| = {bound:.3e} eV; T {src[0, 1]:.1f} -> {src[-1, 1]:.1f} K")
    assert off <= bound, (off, bound)
    assert kept <= bound, (kept, bound)


def test_equilibrate_with_baths_then_drive_with_sources():
    """the usual deck: a run under fix langevin/mdp, unfix, then a run with fix heat/mdp from the state it left"""
    head, hot, cold = _deck("alloy", False)
    text = (_plain(head) + "fix warm mobile langevin/mdp 300.0 300.0 0.05 48271\nrun 50\nunfix warm\n"
            + hot + cold + "thermo_style custom step temp pe ke etotal f_hot f_cold\n" + RUN)
    rc, out, err = _run(text, timeout=600)
    assert rc == 0, err[-3000:]
    rows = _thermo_rows(out)
    first = np.array([r for r in rows if len(r) == 5])
    second = np.array([r for r in rows if len(r) == 7])
    assert first[-1, 0] == 50 and second[0, 0] == 50 and second[-1, 0] == 250
    assert np.ptp(first[:, 4]) > 1e-2                                   # the bath exchanged energy ...
    assert np.all(second[1:, 5] > 1.0) and np.all(second[1:, 6] < 1.0)  # ... and the sources run after it


@pytest.mark.parametrize("other,style", [("fix warm cold langevin/mdp 300.0 300.0 0.05 48271\n", "langevin/mdp")])
def test_a_thermostat_alongside_is_refused_with_both_fixes_named(other, style):
    head, hot, cold = _deck("alloy", False)
    rc, out, err = _run(head.replace(" f_cold", "") + hot + other + RUN, timeout=300)
    assert rc == 1
    assert f"Fix heat/mdp: fix hot cannot run next to fix warm ({style})" in err, err[-2000:]


def test_nvt_mdp_as_the_integrator_is_refused_with_both_fixes_named():
    head, hot, cold = _deck("alloy", False)
    text = head.replace("fix integrate mobile nve/mdp\n", "fix integrate mobile nvt/mdp temp 300.0 300.0 0.1\n").replace(" f_cold", "")
    rc, out, err = _run(text + hot + RUN, timeout=300)
    assert rc == 1
    assert "Fix heat/mdp: fix hot cannot run next to fix integrate (nvt/mdp)" in err, err[-2000:]


def test_without_fix_nve_mdp_the_run_is_refused():
    head, hot, cold = _deck("alloy", False)
    rc, out, err = _run(head.replace("fix integrate mobile nve/mdp\n", "").replace(" f_cold", "") + hot + RUN, timeout=300)
    assert rc == 1 and "Fix heat/mdp requires fix nve/mdp as the time integrator" in err, err[-2000:]
    rc, out, err = _run(head.replace("fix integrate mobile nve/mdp\n", "fix integrate mobile nve\n").replace(" f_cold", "") + hot + RUN,
                        timeout=300)
    # (under LAMMPS `fix nve` is a time_integrate fix and is named as one that integrates on the host; the mini-host's own
    # integrator is no Fix in Modify's list, so there the run misses fix nve/mdp)
    assert rc == 1 and ("integrates on the host" in err or "Fix heat/mdp requires fix nve/mdp" in err), err[-2000:]


def test_two_ranks_are_refused():
    from test_gpu_minilmp_ranks import _double_env
    head, hot, cold = _deck("alloy", False)
    rc, out, err = _run(head.replace(" f_cold", "") + hot + RUN, np=2, env=_double_env(), timeout=300)
    assert rc == 1 and "Fix heat/mdp runs on one MPI rank only" in err, err[-2000:]
