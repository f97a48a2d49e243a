"""GPU: what `init()` and the runs of the four fixes that ride on `fix nve/mdp` share (plugin/fix_rider_mdp.h), through
`plugin load` + `run` in the mini-host on the alloy deck of the plugin tests: a run without fix nve/mdp, one with a host-side
integrator and one with atoms of the fix's group that the integrator does not move are refused, each with its full
sentence; and after a run with the fix and an `unfix`, the next run prints the rows of a deck that never had the fix --
fix nve/mdp switched the feature off in post_run() and cleared what the fix had handed over."""
import pytest

from test_plugin_boundary import _run, _thermo_lines

pytestmark = pytest.mark.gpu

# style -> (plugin file, the fix on GROUP, mode of fix nve/mdp, noun of the held-atoms refusal, what "needs fix nve/mdp")
RIDERS = {
    "langevin/mdp": ("langevinmdpplugin.so", "fix r GROUP langevin/mdp 300.0 300.0 0.05 48271 tally yes\n", "", "thermostat", "the device thermostat needs"),
    "heat/mdp": ("heatmdpplugin.so", "fix r GROUP heat/mdp 1 0.5\n", "", "source", "the device's heat sources need"),
    "indent/mdp": ("indentmdpplugin.so", "fix r GROUP indent/mdp 20.0 sphere 22.2475 22.2475 22.2475 2.4 units box\n", "", None, "the device's indenters need"),
    "spring/mdp": ("springmdpplugin.so", "fix r GROUP spring/mdp tether 5.0 22.0 NULL 20.0 1.0 vel 0.0 0.0 3.0\n", " bricks yes", "spring",
                   "the device's springs need"),
}
STYLES = sorted(RIDERS)
ALLOY = """plugin load aeamplugin.so
plugin load PLUGIN
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
thermo_style custom step temp pe ke etotal
thermo 10
"""


def _parts(style, group="mobile"):
    plugin, fix, mode, noun, needs = RIDERS[style]
    return ALLOY.replace("PLUGIN", plugin), fix.replace("GROUP", group), "fix integrate mobile nve/mdp%s\n" % mode


def _lacking(style):
    return "ERROR: Fix %s requires fix nve/mdp%s as the time integrator (" % (style, " with bricks yes" if style == "spring/mdp" else "")


@pytest.mark.parametrize("style", STYLES)
def test_a_run_without_fix_nve_mdp_is_refused(style):
    head, fix, nve = _parts(style)
    rc, out, err = _run(head + fix + "run 10\n", timeout=300)
    assert rc == 1
    assert _lacking(style) in err, err[-2000:]


@pytest.mark.parametrize("style", STYLES)
def test_a_host_side_integrator_is_refused(style):
    head, fix, nve = _parts(style)
    rc, out, err = _run(head + "fix integrate mobile nve\n" + fix + "run 10\n", timeout=300)
    # (under LAMMPS `fix nve` is a time_integrate fix and is named as one that integrates on the host; the mini-host's own
    # integrator is no Fix in Modify's list, so there the run misses fix nve/mdp)
    on_host = "ERROR: Fix %s: fix integrate (nve) integrates on the host; %s fix nve/mdp as the time integrator (" % (style, RIDERS[style][4])
    assert rc == 1 and (on_host in err or _lacking(style) in err), err[-2000:]


@pytest.mark.parametrize("style", [s for s in STYLES if RIDERS[s][3]])
def test_atoms_the_integrator_does_not_move_are_refused_in_init(style):
    head, fix, nve = _parts(style, group="all")
    rc, out, err = _run(head + fix + nve + "run 10\n", timeout=300)     # (the fix first: its constructor has no integrator to ask)
    assert rc == 1
    assert ("ERROR on proc 0: Fix %s: group all has 1200 atoms outside group mobile of fix integrate (nve/mdp): the %s acts on atoms the "
            "integrator moves (" % (style, RIDERS[style][3])) in err, err[-2000:]


@pytest.mark.parametrize("style", STYLES)
def test_after_an_unfix_the_next_run_is_plain_nve(style):
    head, fix, nve = _parts(style)
    second = "thermo_style custom step temp pe ke etotal\nrun 20\n"
    rc, out, err = _run(head + nve + "run 0\n" + second, timeout=300)
    assert rc == 0, err[-3000:]
    plain = _thermo_lines(out.split("Loop time", 1)[1])
    assert [int(l.split()[0]) for l in plain] == [0, 10, 20]
    rc, out, err = _run(head + nve + fix + "thermo_style custom step temp pe ke etotal f_r\nrun 0\nunfix r\n" + second, timeout=300)
    assert rc == 0, err[-3000:]
    first, rest = out.split("Loop time", 1)
    assert len(_thermo_lines(first)[0].split()) == 6                     # f_r was read in the run that had the fix
    assert _thermo_lines(rest) == plain
