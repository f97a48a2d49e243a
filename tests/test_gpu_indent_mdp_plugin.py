"""GPU: `fix indent/mdp` through `plugin load` + `run` in the mini-host, handing its settings to one `fix nve/mdp` (its
Fix::extract("mdp_indenters") block).  A static sphere on an octahedral site of the alloy under plain `fix nve/mdp`,
host-linked and with `bricks yes`: etotal + f_tip stays flat to ten times what etotal alone keeps in the same deck without
the fix (measured in the same test), while f_tip itself varies by much more.  The shipped sheet example cut to 500 steps:
the load f_tip[3] is zero while the tip is clear of the sheet and positive once it touches, and the held rim has not moved.
Then the refusals that need a run."""
import os

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows

pytestmark = pytest.mark.gpu
A0 = 4.045

ALLOY = """plugin load aeamplugin.so
plugin load indentmdpplugin.so
plugin load heatmdpplugin.so
plugin load nvtmdpplugin.so
plugin load minimizemdpplugin.so
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
group substrate region floor
group mobile subtract all substrate
timestep 0.001
velocity all create 300.0 1082337
velocity substrate set 0.0 0.0 0.0
fix integrate mobile nve/mdp
thermo_style custom step temp pe ke etotal f_tip f_tip[1] f_tip[2] f_tip[3]
thermo 10
"""
# an octahedral site between the mobile layers: six neighbours at a / 2 = 2.02 A, 0.38 A inside the sphere
TIP = f"fix tip all indent/mdp 20.0 sphere {5.5 * A0} {5.5 * A0} {5.5 * A0} 2.4 units box\n"
RUN = "run 200\n"
COLS = " f_tip f_tip[1] f_tip[2] f_tip[3]"


def _rows(script, nrows=21, last=200):
    rc, out, err = _run(script, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert len(rows) == nrows and rows[-1, 0] == last, rows
    return rows


@pytest.mark.parametrize("bricks", [False, True], ids=["host-linked", "bricks"])
def test_a_static_indenter_keeps_etotal_plus_its_energy(bricks, capsys):
    deck = ALLOY.replace("nve/mdp\n", "nve/mdp bricks yes\n") if bricks else ALLOY
    plain = _rows(deck.replace(COLS, "") + RUN)
    bound = float(np.abs(plain[:, 4] - plain[0, 4]).max())
    rows = _rows(deck + TIP + RUN)
    total = rows[:, 4] + rows[:, 5]
    kept = float(np.abs(total - total[0]).max())
    swing = float(np.ptp(rows[:, 5]))
    with capsys.disabled():
        print(f"indent/mdp alloy, {'bricks yes' if bricks else 'host-linked'}: etotal + f_tip moved by {kept:.3e} eV, f_tip alone spans "
              f"{swing:.3e} eV ({rows[0, 5]:.4f} at step 0); max|dE| of the deck without the fix {bound:.3e} eV")
    assert bound > 0.0
    assert kept <= 10.0 * bound, (kept, bound)
    assert swing > 10.0 * bound, (swing, bound)
    assert rows[0, 5] > 1.0                                             # six atoms stand 0.38 A inside the sphere at step 0
    on = rows[:, 5] > 0.0
    assert np.all(np.abs(rows[on, 6:9]).max(axis=1) > 0.0) and not rows[~on, 6:9].any()   # whoever touches it pushes on it


def test_the_two_modes_print_the_same_columns():
    a = _rows(ALLOY + TIP + RUN)
    b = _rows(ALLOY.replace("nve/mdp\n", "nve/mdp bricks yes\n") + TIP + RUN)
    for c in (1, 2, 3, 4, 5):
        assert np.allclose(a[:, c], b[:, c], rtol=2e-7, atol=1e-9), (c, a[:, c], b[:, c])
    for c in (6, 7, 8):                                                 # sums of six terms of either sign
        assert np.allclose(a[:, c], b[:, c], rtol=2e-7, atol=1e-6), (c, a[:, c], b[:, c])


def test_a_second_run_starts_the_centre_again_and_its_setup_row_is_read_anew():
    """two runs of a sphere that moves 0.4 A per 100 steps: the row of step 100 that closes the first run has the centre
    0.4 A along, the row of step 100 that opens the second has it back at c -- the fix reads the state once per step and
    must not hand the second run the first run's last read"""
    tip = TIP.replace(" units box", " vel 0.0 0.0 4.0 units box")
    assert tip != TIP
    rc, out, err = _run(ALLOY.replace("thermo 10\n", "thermo 100\n") + tip + "run 100\nrun 100\n", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(r) for r in rows[:, 0]] == [0, 100, 100, 200]
    assert rows[0, 5] > 1.0 and rows[1, 5] > 0.0                        # (0.4 A nearer its upper neighbour, the sphere holds it)
    assert rows[1, 5] != rows[2, 5] and not np.array_equal(rows[1, 6:9], rows[2, 6:9])
    # the four columns of a row come from one read: the force is that of the row's own energy (both zero or neither)
    assert np.array_equal(rows[:, 5] > 0.0, np.abs(rows[:, 6:9]).max(axis=1) > 0.0)


def test_the_sheet_example_the_load_comes_on_at_contact_and_the_rim_stays(tmp_path, capsys):
    text = open(os.path.join(PKG, "examples", "in.rebomos-sheet.indent-mdp.mi355x")).read()
    tip = "fix tip all indent/mdp 10.0 sphere 19.15 22.12 22.31 8.0 vel 0.0 0.0 -4.0 units box\n"
    assert tip in text and "thermo_style custom step temp pe ke etotal f_tip f_tip[3]" in text and "run 1000" in text
    assert "fix warm bath langevin/mdp" in text and "fix integrate mobile nve/mdp" in text
    text = text.replace("run 1000", "run 500").replace("thermo 100\n", f"thermo 50\nwrite_dump rim custom {tmp_path / 'before'} id x y z vx vy vz\n")
    text = text.replace("write_dump rim custom rim.dump", f"write_dump rim custom {tmp_path / 'after'}")
    rc, out, err = _run(text, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(r) for r in rows[:, 0]] == list(range(0, 501, 50))
    load, energy = rows[:, 6], rows[:, 5]
    with capsys.disabled():
        print("sheet example, load f_tip[3] by step: " + " ".join(f"{int(n)}:{l:.4g}" for n, l in zip(rows[:, 0], load)))
    # the tip's lowest point starts 1 A above the top sulphur plane and comes down 0.2 A per 50 steps: 0.6 A clear of the
    # plane's rest position at step 100, which thermal motion at 300 K does not bridge, and 1 A into it at the end
    assert np.all(load[:3] == 0.0) and np.all(energy[:3] == 0.0), load
    assert load[-1] > 0.0 and energy[-1] > 0.0, load
    assert np.all(load >= 0.0)
    touched = np.flatnonzero(load > 0.0)
    assert len(touched) >= 2 and np.all(load[touched[0]:] > 0.0)        # once it touches it stays in touch
    before = (tmp_path / "before").read_text().splitlines()[5:]
    after = (tmp_path / "after").read_text().splitlines()[5:]
    assert len(before) > 100 and before == after                        # the held rim: digit for digit


def test_nvt_mdp_as_the_integrator_is_refused_with_both_fixes_named():
    text = ALLOY.replace("fix integrate mobile nve/mdp\n", "fix integrate mobile nvt/mdp temp 300.0 300.0 0.1\n")
    rc, out, err = _run(text + TIP + RUN, timeout=300)
    assert rc == 1
    assert "Fix indent/mdp: fix tip cannot run next to fix integrate (nvt/mdp)" in err, err[-2000:]


def test_heat_mdp_alongside_is_refused_with_both_fixes_named():
    rc, out, err = _run(ALLOY + TIP + "fix hot mobile heat/mdp 1 0.5\n" + RUN, timeout=300)
    assert rc == 1
    assert "Fix indent/mdp: fix tip cannot run next to fix hot (heat/mdp)" in err, err[-2000:]


def test_without_fix_nve_mdp_the_run_is_refused():
    rc, out, err = _run(ALLOY.replace("fix integrate mobile nve/mdp\n", "") + TIP + RUN, timeout=300)
    assert rc == 1 and "Fix indent/mdp requires fix nve/mdp as the time integrator" in err, err[-2000:]


def test_minimize_mdp_refuses_to_run_over_an_indenter():
    rc, out, err = _run(ALLOY + TIP + "minimize/mdp 0.0 1.0e-4 100 1000\n", timeout=300)
    assert rc == 1
    assert "minimize/mdp: fix tip (indent/mdp) is not applied by the minimiser; unfix it first" in err, err[-2000:]


def test_two_ranks_are_refused():
    from test_gpu_minilmp_ranks import _double_env
    rc, out, err = _run(ALLOY + TIP + RUN, np=2, env=_double_env(), timeout=300)
    assert rc == 1 and "Fix indent/mdp runs on one MPI rank only" in err, err[-2000:]
