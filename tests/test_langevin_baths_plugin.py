"""CPU: several `fix langevin/mdp` at the plugin boundary.  Two, three and four of them on disjoint groups are accepted; a
fifth is refused, and so are two whose groups share atoms -- with both fix IDs and the number of shared atoms -- before a
device is touched (the constructor looks at the langevin/mdp fixes defined so far; init() looks again at run time)."""
import pytest

from test_plugin_boundary import HEAD, _run

LOAD = "plugin load langevinmdpplugin.so\n" + HEAD
# 2 x 2 x 2 fcc cells, 32 atoms in layers of 8 (tests/test_group_mdp_plugin.py): four disjoint z layers, and two that overlap
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
group few id 1:3
"""
HOT = "fix hot g0 langevin/mdp 900.0 900.0 0.05 48271 tally yes\n"
COLD = "fix cold g1 langevin/mdp 100.0 100.0 0.02 7919 tally yes zero yes\n"
WARM = "fix warm g2 langevin/mdp 300.0 600.0 0.1 48271 scale 1 2.0\n"
MILD = "fix mild g3 langevin/mdp 300.0 300.0 0.1 11\n"


def test_the_layers_are_disjoint_groups_of_eight():
    rc, out, err = _run(GROUPS)
    assert rc == 0, err
    for g in ("g0", "g1", "g2", "g3"):
        assert f"8 atoms in group {g}" in out, out
    assert "16 atoms in group bottom" in out


@pytest.mark.parametrize("fixes", [HOT + COLD, HOT + COLD + WARM, COLD + WARM + HOT + MILD], ids=["two", "three", "four"])
def test_several_baths_on_disjoint_groups_parse(fixes):
    rc, out, err = _run(GROUPS + fixes)
    assert rc == 0, err
    assert "ERROR" not in err


def test_a_fifth_bath_is_refused():
    rc, out, err = _run(GROUPS + HOT + COLD + WARM + MILD + "fix fifth few langevin/mdp 300.0 300.0 0.1 12\n")
    assert rc == 1
    assert "fifth is langevin/mdp fix number 5; fix nve/mdp takes up to 4 of them" in err, err


def test_a_bath_may_be_replaced_after_unfix():
    rc, out, err = _run(GROUPS + HOT + COLD + WARM + MILD + "unfix warm\nfix again g2 langevin/mdp 300.0 300.0 0.1 12\n")
    assert rc == 0, err


@pytest.mark.parametrize("second,ids,count", [
    ("fix cold bottom langevin/mdp 100.0 100.0 0.02 7919\n", "fixes hot and cold share 8 atoms (groups g0 and bottom)", 8),
    ("fix cold all langevin/mdp 100.0 100.0 0.02 7919\n", "fixes hot and cold share 8 atoms (groups g0 and all)", 8),
    ("fix cold g0 langevin/mdp 100.0 100.0 0.02 7919\n", "fixes hot and cold share 8 atoms (groups g0 and g0)", 8),
])
def test_overlapping_groups_are_refused_and_both_fixes_are_named(second, ids, count):
    rc, out, err = _run(GROUPS + HOT + second)
    assert rc == 1
    assert ids in err and "must be disjoint" in err, err


def test_the_overlap_is_found_behind_a_disjoint_bath_too():
    rc, out, err = _run(GROUPS + HOT + COLD + "fix third bottom langevin/mdp 300.0 300.0 0.1 12\n")
    assert rc == 1
    assert "fixes hot and third share 8 atoms" in err, err
