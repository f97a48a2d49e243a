"""CPU: what the four fixes that ride on `fix nve/mdp` share (plugin/fix_rider_mdp.h) -- fix langevin/mdp, fix heat/mdp,
fix indent/mdp and fix spring/mdp on the 32-atom cell of test_plugin_boundary.  The group refusals and the refusal of a fifth
fix are one sentence each with the style's name in it; a fix that re-uses the ID of an existing one replaces it, so it is
neither counted as a fifth nor, for the two styles whose groups must be disjoint, refused for sharing atoms with itself."""
import pytest

from test_plugin_boundary import HEAD, _run

# style -> (plugin file, arguments behind the style's name, what an empty group leaves out)
RIDERS = {
    "langevin/mdp": ("langevinmdpplugin.so", "300.0 300.0 0.05 48271", "there is no atom to thermostat"),
    "heat/mdp": ("heatmdpplugin.so", "1 0.5", "there is no atom to heat"),
    "indent/mdp": ("indentmdpplugin.so", "5.0 sphere 1.0 1.0 1.0 1.0 units box", "there is no atom to push on"),
    "spring/mdp": ("springmdpplugin.so", "tether 5.0 1.0 1.0 1.0 0.0", "there is no centre of mass to pull on"),
}
STYLES = sorted(RIDERS)
# four disjoint z layers of 8 atoms (tests/test_heat_mdp_plugin.py) and a group without atoms
GROUPS = """region l0 block 0 2 0 2 0 0.2
region l1 block 0 2 0 2 0.4 0.6
region l2 block 0 2 0 2 0.9 1.1
region l3 block 0 2 0 2 1.4 1.6
group g0 region l0
group g1 region l1
group g2 region l2
group g3 region l3
group silicon type 2
"""


def _deck(style):
    return "plugin load rebomosplugin.so\nplugin load %s\n" % RIDERS[style][0] + HEAD + GROUPS


def _fix(style, fid, group):
    return "fix %s %s %s %s\n" % (fid, group, style, RIDERS[style][1])


def _four(style):
    return "".join(_fix(style, fid, g) for fid, g in (("a", "g0"), ("b", "g1"), ("c", "g2"), ("d", "g3")))


@pytest.mark.parametrize("style", STYLES)
def test_an_unknown_group_is_refused(style):
    rc, out, err = _run(_deck(style) + _fix(style, "f", "nosuch"))
    assert rc == 1
    assert "ERROR: Fix %s requires group all or a group defined by the group command: could not find fix group ID nosuch (" % style in err, err


@pytest.mark.parametrize("style", STYLES)
def test_an_empty_group_is_refused(style):
    rc, out, err = _run(_deck(style) + _fix(style, "f", "silicon"))
    assert rc == 1
    assert "ERROR: Fix %s: group silicon is empty: %s (" % (style, RIDERS[style][2]) in err, err


@pytest.mark.parametrize("style", STYLES)
def test_four_are_accepted_and_a_fifth_is_refused(style):
    rc, out, err = _run(_deck(style) + _four(style))
    assert rc == 0 and "ERROR" not in err, err
    rc, out, err = _run(_deck(style) + _four(style) + _fix(style, "fifth", "g0"))
    assert rc == 1
    assert "ERROR: Fix %s: fifth is %s fix number 5; fix nve/mdp takes up to 4 of them (" % (style, style) in err, err


@pytest.mark.parametrize("style", STYLES)
def test_a_fix_with_the_id_of_the_fourth_replaces_it(style):
    rc, out, err = _run(_deck(style) + _four(style) + _fix(style, "d", "g3"))
    assert rc == 0 and "ERROR" not in err, err


@pytest.mark.parametrize("style,fid", [("heat/mdp", "hot"), ("langevin/mdp", "warm")])
def test_a_fix_issued_twice_under_one_id_does_not_share_atoms_with_itself(style, fid):
    rc, out, err = _run(_deck(style) + _fix(style, fid, "g0") + _fix(style, fid, "g0"))
    assert rc == 0 and "ERROR" not in err, err
    # ... and atoms shared with another fix of the style are refused as before
    rc, out, err = _run(_deck(style) + _fix(style, fid, "g0") + _fix(style, "other", "g0"))
    assert rc == 1
    assert "ERROR: Fix %s: fixes %s and other share 8 atoms (groups g0 and g0); the groups of several %s fixes must be disjoint (" % (style, fid, style) in err, err
