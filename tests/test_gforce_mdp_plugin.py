"""CPU: `fix setforce/mdp`, `fix addforce/mdp` and `fix aveforce/mdp` at the plugin boundary.  One plugin file registers the
three styles; `fx fy fz` parse in LAMMPS' argument order, NULL included where the style takes it; the three styles are one
family that shares four slots, and a fix that re-uses an ID is not a fifth.  Everything the constructors refuse is refused
before a device is touched, with a message naming the problem.  The plugin object exports the one symbol `plugin load`
looks up; the mini-host takes f_ID and f_ID[1..3] as thermo columns."""
import os
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load rebomosplugin.so\nplugin load gforcemdpplugin.so\n" + HEAD
GROUPS = LOAD + """region l0 block 0 2 0 2 0 0.2
region low block 0 2 0 2 0 0.6
group g0 region l0
group bottom region low
group silicon type 2
"""
GRIP = "fix grip g0 setforce/mdp 0.0 0.0 0.0\n"
STYLES = ("setforce/mdp", "addforce/mdp", "aveforce/mdp")


def test_the_plugin_loads_and_registers_three_styles():
    rc, out, err = _run(GROUPS + GRIP + "fix body all addforce/mdp 0.0 0.0 -0.01\nfix load bottom aveforce/mdp NULL NULL -0.5\n")
    assert rc == 0, err
    assert "Loaded 3 plugins from gforcemdpplugin.so" in out


def test_the_plugin_object_exports_one_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "gforcemdpplugin.so")], capture_output=True, text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]


@pytest.mark.parametrize("args", [
    "g0 setforce/mdp 0.0 0.0 0.0",
    "all setforce/mdp NULL NULL NULL",
    "bottom setforce/mdp 0 0 NULL",
    "g0 setforce/mdp 1e-1 NULL -2.5",
    "all addforce/mdp 0.0 0.0 -0.01",
    "g0 addforce/mdp 1.5e-2 -3 0",
    "bottom aveforce/mdp NULL NULL -0.5",
    "all aveforce/mdp 0.0 0.0 0.0",
    "g0 aveforce/mdp NULL NULL NULL",
])
def test_the_argument_forms_parse(args):
    rc, out, err = _run(GROUPS + "fix f " + args + "\n")
    assert rc == 0, err
    assert "ERROR" not in err


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("args,msg", [
    ("nosuch {s} 0 0 0", "Fix {s} requires group all or a group defined by the group command: could not find fix group ID nosuch"),
    ("silicon {s} 0 0 0", "Fix {s}: group silicon is empty: there is no atom to act on"),
    ("all {s}", "Illegal fix {s} command: fix ID group {s} fx fy fz"),
    ("all {s} 0 0", "Illegal fix {s} command: fix ID group {s} fx fy fz"),
    ("all {s} v_fx 0 0", "Fix {s}: a variable as an argument is not supported (v_fx); the values are constants"),
    ("all {s} 0 0 v_fz", "Fix {s}: a variable as an argument is not supported (v_fz)"),
    ("all {s} 0 0 0 region v_r", "Fix {s}: a variable as an argument is not supported (v_r)"),
    ("all {s} 0 v_fy", "Fix {s}: a variable as an argument is not supported (v_fy)"),
    ("all {s} 0 0 0 region l0", "Fix {s}: region is not supported; the fix acts on every atom of its group"),
    ("all {s} much 0 0", "Illegal fix {s} command: bad fx value much"),
    ("all {s} 0 inf 0", "Illegal fix {s} command: bad fy value inf"),
    ("all {s} 0 0 nan", "Illegal fix {s} command: bad fz value nan"),
    ("all {s} 0 0 null", "Illegal fix {s} command: bad fz value null"),
    ("all {s} 0 0 0 often", "Illegal fix {s} command: unknown keyword often"),
    ("all {s} 0 0 0 0", "Illegal fix {s} command: unknown keyword 0"),
])
def test_constructor_refusals_of_all_three_styles(style, args, msg):
    rc, out, err = _run(GROUPS + "fix f " + args.format(s=style) + "\n")
    assert rc == 1
    assert msg.format(s=style) in err, err


@pytest.mark.parametrize("args,msg", [
    ("all addforce/mdp NULL 0 0", "Fix addforce/mdp: fx is NULL; addforce takes three numbers"),
    ("all addforce/mdp 0 0 NULL", "Fix addforce/mdp: fz is NULL; addforce takes three numbers"),
    ("all addforce/mdp 0 0 0.1 every 10", "Fix addforce/mdp: every is not supported; the force is added on every step and is constant"),
    ("all addforce/mdp 0 0 0.1 energy v_e", "Fix addforce/mdp: a variable as an argument is not supported (v_e)"),
    ("all addforce/mdp 0 0 0.1 energy e", "Fix addforce/mdp: energy is not supported"),
    ("all setforce/mdp 0 0 0.1 every 10", "Illegal fix setforce/mdp command: unknown keyword every"),
    ("all aveforce/mdp 0 0 0.1 energy e", "Illegal fix aveforce/mdp command: unknown keyword energy"),
])
def test_constructor_refusals_of_one_style(args, msg):
    rc, out, err = _run(GROUPS + "fix f " + args + "\n")
    assert rc == 1
    assert msg in err, err


def test_the_family_shares_four_slots_and_a_fifth_fix_is_refused():
    four = (GRIP + "fix body all addforce/mdp 0.0 0.0 -0.01\nfix flat bottom setforce/mdp 0 0 NULL\n"
            "fix load bottom aveforce/mdp NULL NULL -0.5\n")
    rc, out, err = _run(GROUPS + four)
    assert rc == 0, err
    for style in STYLES:
        rc, out, err = _run(GROUPS + four + f"fix fifth g0 {style} 0.0 0.0 0.0\n")
        assert rc == 1
        assert (f"Fix {style}: fifth is setforce/mdp, addforce/mdp or aveforce/mdp fix number 5; fix nve/mdp takes up to 4 of them") in err, err
    rc, out, err = _run(GROUPS + four + "unfix body\nfix again g0 aveforce/mdp 0.1 NULL NULL\n")
    assert rc == 0, err
    # a fix with the ID of one of the four replaces it, whatever its style: it is not a fifth
    rc, out, err = _run(GROUPS + four + "fix body g0 setforce/mdp NULL 0.0 NULL\n")
    assert rc == 0, err


@pytest.mark.parametrize("cols", ["step f_grip[1]", "step f_grip[1] f_grip[2] f_grip[3] f_body f_body[3] etotal"])
def test_the_scalar_and_the_three_vector_columns_are_accepted(cols):
    rc, out, err = _run(GROUPS + GRIP + "fix body all addforce/mdp 0.0 0.0 -0.01\n" + f"thermo_style custom {cols}\n")
    assert rc == 0, err


@pytest.mark.parametrize("col", ["f_grip[0]", "f_grip[4]"])
def test_an_index_outside_the_vector_is_refused(col):
    rc, out, err = _run(GROUPS + GRIP + f"thermo_style custom step {col}\n")
    assert rc == 1
    assert f"Thermo custom fix grip is a vector of 3: {col} is not one of its elements" in err, err


def test_the_capi_holds_the_four_names():
    from lammps_plugins_amd.host import capi
    assert {"mdp_gforce_setup", "mdp_gforce_run", "mdp_gforce_state", "mdp_gforce_off"} <= set(capi.EXPORTS)
    assert (capi.GFORCE_MAX, capi.GFORCE_STATE_LEN) == (4, 10)


def test_the_example_inputs_are_there_and_name_what_the_gpu_test_runs():
    text = open(os.path.join(PKG, "examples", "in.rebomos-ribbon.tensile-mdp.mi355x")).read()
    assert "fix integrate mobile nve/mdp" in text and "fix warm strip langevin/mdp" in text
    assert "velocity grip set 0.0 0.5 0.0" in text and "fix grip grip setforce/mdp 0.0 0.0 0.0" in text
    assert "thermo_style custom step temp pe ke etotal f_grip[1] f_grip[2]" in text
    text = open(os.path.join(PKG, "examples", "in.rebomos-bilayer.load-mdp.mi355x")).read()
    assert "fix flat top setforce/mdp 0.0 0.0 NULL" in text and "fix load top aveforce/mdp NULL NULL -0.05" in text
    assert "thermo_style custom step temp pe ke etotal f_flat[1] f_load[3]" in text
