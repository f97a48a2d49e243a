"""CPU: `fix spring/mdp` at the plugin boundary.  `tether K x y z R0 [vel vx vy vz]` parses in LAMMPS' argument order, NULL
included; up to four fixes are accepted, on groups that may share atoms, and a fix that re-uses an ID is not a fifth.
Everything the constructor refuses is refused before a device is touched, with a message naming the problem.  The plugin
object exports the one symbol `plugin load` looks up; the mini-host takes f_ID and f_ID[1..4] as thermo columns."""
import os
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load rebomosplugin.so\nplugin load springmdpplugin.so\n" + HEAD
GROUPS = LOAD + """region l0 block 0 2 0 2 0 0.2
region low block 0 2 0 2 0 0.6
group g0 region l0
group bottom region low
group silicon type 2
"""
PULL = "fix pull all spring/mdp tether 5.0 4.0 NULL NULL 0.0 vel 2.0 0.0 0.0\n"


def test_the_plugin_loads_and_registers_one_style():
    rc, out, err = _run(GROUPS + PULL)
    assert rc == 0, err
    assert "Loaded 1 plugins from springmdpplugin.so" in out


def test_the_plugin_object_exports_one_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "springmdpplugin.so")], capture_output=True, text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]


@pytest.mark.parametrize("args", [
    "all spring/mdp tether 5.0 4.0 4.0 4.0 0.0",
    "g0 spring/mdp tether 5.0 4.0 4.0 4.0 2.5",
    "g0 spring/mdp tether 0.0 NULL 4.0 4.0 1.0",
    "bottom spring/mdp tether 5.0 NULL NULL -4.0 0.0 vel 0.0 0.0 1.5",
    "all spring/mdp tether 5.0 4.0 NULL NULL 0.0 vel 2.0 7.0 -7.0",
    "all spring/mdp tether 5e-1 4.0 NULL 1.0e1 0.25 vel -2.0 0.0 0.0",
])
def test_the_argument_forms_parse(args):
    rc, out, err = _run(GROUPS + "fix pull " + args + "\n")
    assert rc == 0, err
    assert "ERROR" not in err


@pytest.mark.parametrize("args,msg", [
    ("nosuch spring/mdp tether 5.0 4 4 4 0.0", "Fix spring/mdp requires group all or a group defined by the group command: could not find fix group ID nosuch"),
    ("silicon spring/mdp tether 5.0 4 4 4 0.0", "Fix spring/mdp: group silicon is empty"),
    ("all spring/mdp", "Illegal fix spring/mdp command"),
    ("all spring/mdp tether 5.0 4 4 4", "Illegal fix spring/mdp command"),
    ("all spring/mdp couple g0 5.0 4 4 4 0.0", "Fix spring/mdp: couple is not supported; only tether is"),
    ("all spring/mdp pull 5.0 4 4 4 0.0", "Illegal fix spring/mdp command: unknown mode pull"),
    ("all spring/mdp tether v_k 4 4 4 0.0", "Fix spring/mdp: a variable as an argument is not supported (v_k)"),
    ("all spring/mdp tether 5.0 v_x 4 4 0.0", "Fix spring/mdp: a variable as an argument is not supported (v_x)"),
    ("all spring/mdp tether 5.0 4 4 4 v_r", "a variable as an argument is not supported (v_r); a moving tether point takes vel vx vy vz"),
    ("all spring/mdp tether 5.0 4 4 4 0.0 vel 0 0 v_z", "Fix spring/mdp: a variable as an argument is not supported (v_z)"),
    ("all spring/mdp tether much 4 4 4 0.0", "Illegal fix spring/mdp command: bad K value much"),
    ("all spring/mdp tether -1.0 4 4 4 0.0", "Fix spring/mdp: K must be >= 0.0"),
    ("all spring/mdp tether inf 4 4 4 0.0", "Illegal fix spring/mdp command: bad K value inf"),
    ("all spring/mdp tether 5.0 4 4 4 -0.5", "Fix spring/mdp: R0 must be >= 0.0"),
    ("all spring/mdp tether 5.0 4 4 4 long", "Illegal fix spring/mdp command: bad R0 value long"),
    ("all spring/mdp tether 5.0 4 far 4 0.0", "Illegal fix spring/mdp command: bad y value far"),
    ("all spring/mdp tether 5.0 4 null 4 0.0", "Illegal fix spring/mdp command: bad y value null"),
    ("all spring/mdp tether 5.0 NULL NULL NULL 0.0", "Fix spring/mdp: x, y and z are all NULL"),
    ("all spring/mdp tether 5.0 4 4 4 0.0 vel 0 0", "Illegal fix spring/mdp command: vel needs vx vy vz"),
    ("all spring/mdp tether 5.0 4 4 4 0.0 often", "Illegal fix spring/mdp command: unknown keyword often"),
    ("all spring/mdp tether 5.0 4 4 4 0.0 units box", "Illegal fix spring/mdp command: unknown keyword units"),
])
def test_constructor_refusals(args, msg):
    rc, out, err = _run(GROUPS + "fix pull " + args + "\n")
    assert rc == 1
    assert msg in err, err


def test_four_springs_may_share_atoms_and_a_fifth_is_refused():
    four = PULL + "".join(f"fix s{k} {g} spring/mdp tether 5.0 NULL NULL {k}.0 0.5\n" for k, g in enumerate(("g0", "bottom", "all")))
    rc, out, err = _run(GROUPS + four)
    assert rc == 0, err
    rc, out, err = _run(GROUPS + four + "fix fifth g0 spring/mdp tether 5.0 1.0 NULL NULL 0.0\n")
    assert rc == 1
    assert "fifth is spring/mdp fix number 5; fix nve/mdp takes up to 4 of them" in err, err
    rc, out, err = _run(GROUPS + four + "unfix s1\nfix again g0 spring/mdp tether 5.0 1.0 NULL NULL 0.0\n")
    assert rc == 0, err
    # a fix with the ID of one of the four replaces it: it is not a fifth
    rc, out, err = _run(GROUPS + four + "fix s1 g0 spring/mdp tether 7.0 1.0 NULL NULL 0.0\n")
    assert rc == 0, err


@pytest.mark.parametrize("cols", ["step f_pull", "step f_pull f_pull[1] f_pull[2] f_pull[3] f_pull[4] etotal"])
def test_the_scalar_and_the_four_vector_columns_are_accepted(cols):
    rc, out, err = _run(GROUPS + PULL + f"thermo_style custom {cols}\n")
    assert rc == 0, err


@pytest.mark.parametrize("col", ["f_pull[0]", "f_pull[5]"])
def test_an_index_outside_the_vector_is_refused(col):
    rc, out, err = _run(GROUPS + PULL + f"thermo_style custom step {col}\n")
    assert rc == 1
    assert f"Thermo custom fix pull is a vector of 4: {col} is not one of its elements" in err, err


def test_the_capi_holds_the_four_names():
    from lammps_plugins_amd.host import capi
    assert {"mdp_spring_setup", "mdp_spring_run", "mdp_spring_state", "mdp_spring_off"} <= set(capi.EXPORTS)


def test_the_example_input_is_there_and_names_what_the_gpu_test_runs():
    text = open(os.path.join(PKG, "examples", "in.rebomos-bilayer.spring-mdp.mi355x")).read()
    assert "fix integrate mobile nve/mdp bricks yes" in text and "fix warm bath langevin/mdp" in text
    assert "fix pull upper spring/mdp tether 5.0 19.46 NULL NULL 0.0 vel 2.0 0.0 0.0" in text
    assert "thermo_style custom step temp pe ke etotal f_pull f_pull[1] f_pull[4]" in text
