"""CPU: `fix heat/mdp` at the plugin boundary.  Up to four on disjoint groups are accepted; everything its constructor
refuses is refused before a device is touched, with a message naming the problem: an unknown or empty group, N < 1, a
variable as eflux, the region keyword, a fifth heat/mdp, groups that share atoms with an earlier heat/mdp (both IDs, the
count) and atoms the integrator does not move."""
import pytest

from test_plugin_boundary import HEAD, _run

LOAD = "plugin load rebomosplugin.so\nplugin load heatmdpplugin.so\n" + HEAD
# 2 x 2 x 2 fcc cells, 32 atoms in layers of 8 (tests/test_langevin_baths_plugin.py): four disjoint z layers, and two that overlap
GROUPS = LOAD + """region l0 block 0 2 0 2 0 0.2
region l1 block 0 2 0 2 0.4 0.6
region l2 block 0 2 0 2 0.9 1.1
region l3 block 0 2 0 2 1.4 1.6
region low block 0 2 0 2 0 0.6
group g0 region l0
group g1 region l1
group g2 region l2
group g3 region l3
group bottom region low
group upper subtract all bottom
group silicon type 2
group few id 1:3
"""
HOT = "fix hot g0 heat/mdp 1 0.5\n"
COLD = "fix cold g1 heat/mdp 1 -0.5\n"
WARM = "fix warm g2 heat/mdp 3 1.0e-2\n"
MILD = "fix mild g3 heat/mdp 10 -1.0e-2\n"


def test_the_plugin_loads_and_the_fix_parses():
    rc, out, err = _run(GROUPS + HOT)
    assert rc == 0, err
    assert "Loaded 1 plugins from heatmdpplugin.so" in out


@pytest.mark.parametrize("fixes", [HOT + COLD, HOT + COLD + WARM, COLD + WARM + HOT + MILD], ids=["two", "three", "four"])
def test_several_sources_on_disjoint_groups_parse(fixes):
    rc, out, err = _run(GROUPS + fixes)
    assert rc == 0, err
    assert "ERROR" not in err


@pytest.mark.parametrize("args,msg", [
    ("nosuch heat/mdp 1 0.5", "Fix heat/mdp requires group all or a group defined by the group command: could not find fix group ID nosuch"),
    ("silicon heat/mdp 1 0.5", "Fix heat/mdp: group silicon is empty"),
    ("g0 heat/mdp 1", "Illegal fix heat/mdp command"),
    ("g0 heat/mdp 0 0.5", "Fix heat/mdp: N must be >= 1"),
    ("g0 heat/mdp -2 0.5", "Fix heat/mdp: N must be >= 1"),
    ("g0 heat/mdp 1.5 0.5", "Illegal fix heat/mdp command: bad N value 1.5"),
    ("g0 heat/mdp 1 v_flux", "Fix heat/mdp: a variable as eflux is not supported (v_flux)"),
    ("g0 heat/mdp 1 much", "Illegal fix heat/mdp command: bad eflux value much"),
    ("g0 heat/mdp 1 inf", "Illegal fix heat/mdp command: bad eflux value inf"),
    ("g0 heat/mdp 1 0.5 region l0", "Fix heat/mdp: keyword region is not supported"),
    ("g0 heat/mdp 1 0.5 often", "Illegal fix heat/mdp command: unknown keyword often"),
])
def test_constructor_refusals(args, msg):
    rc, out, err = _run(GROUPS + "fix hot " + args + "\n")
    assert rc == 1
    assert msg in err, err


def test_a_fifth_source_is_refused():
    rc, out, err = _run(GROUPS + HOT + COLD + WARM + MILD + "fix fifth few heat/mdp 1 0.1\n")
    assert rc == 1
    assert "fifth is heat/mdp fix number 5; fix nve/mdp takes up to 4 of them" in err, err


def test_a_source_may_be_replaced_after_unfix():
    rc, out, err = _run(GROUPS + HOT + COLD + WARM + MILD + "unfix warm\nfix again g2 heat/mdp 1 0.1\n")
    assert rc == 0, err


@pytest.mark.parametrize("second,ids", [
    ("fix cold bottom heat/mdp 1 -0.5\n", "fixes hot and cold share 8 atoms (groups g0 and bottom)"),
    ("fix cold all heat/mdp 1 -0.5\n", "fixes hot and cold share 8 atoms (groups g0 and all)"),
    ("fix cold g0 heat/mdp 1 -0.5\n", "fixes hot and cold share 8 atoms (groups g0 and g0)"),
])
def test_overlapping_groups_are_refused_and_both_fixes_are_named(second, ids):
    rc, out, err = _run(GROUPS + HOT + second)
    assert rc == 1
    assert ids in err and "must be disjoint" in err, err


def test_the_overlap_is_found_behind_a_disjoint_source_too():
    rc, out, err = _run(GROUPS + HOT + COLD + "fix third bottom heat/mdp 1 0.1\n")
    assert rc == 1
    assert "fixes hot and third share 8 atoms" in err, err


@pytest.mark.parametrize("cmds,msg", [
    ("fix 1 upper nve/mdp\nfix hot g1 heat/mdp 1 0.5", "Fix heat/mdp: group g1 has 8 atoms outside group upper of fix 1 (nve/mdp)"),
    ("fix 1 upper nve/mdp\nfix hot all heat/mdp 1 0.5", "Fix heat/mdp: group all has 16 atoms outside group upper of fix 1 (nve/mdp)"),
])
def test_atoms_the_integrator_does_not_move_are_refused(cmds, msg):
    rc, out, err = _run(GROUPS + cmds + "\n")
    assert rc == 1
    assert msg in err, err
    rc, out, err = _run(GROUPS + "fix 1 upper nve/mdp\nfix hot g2 heat/mdp 1 0.5\nfix cold g3 heat/mdp 1 -0.5\n")
    assert rc == 0, err
