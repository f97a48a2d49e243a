"""CPU: `fix langevin/mdp` at the plugin boundary -- langevinmdpplugin.so exports the one C symbol `plugin load` looks
up, registers one style, and refuses bad input with a message naming the problem before a device is touched."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load langevinmdpplugin.so\n" + HEAD


def test_langevin_plugin_exports_only_lammpsplugin_init_and_holds_the_fix():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "langevinmdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS14FixLangevinMDP14compute_scalarEv", out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


def test_langevin_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "fix 2 all langevin/mdp 300.0 300.0 0.1 48271\n")
    assert rc == 0, err
    assert "Loaded 1 plugins from langevinmdpplugin.so" in out


@pytest.mark.parametrize("args,msg", [
    ("mobile langevin/mdp 300 300 0.1 48271", "requires group all"),
    ("all langevin/mdp 300 300 0.1", "Illegal fix langevin/mdp command"),
    ("all langevin/mdp v_t 300 0.1 48271", "variables are not supported"),
    ("all langevin/mdp 300 v_t 0.1 48271", "variables are not supported"),
    ("all langevin/mdp 300 300 0.0 48271", "damp must be > 0.0"),
    ("all langevin/mdp 300 300 -0.1 48271", "damp must be > 0.0"),
    ("all langevin/mdp -1 300 0.1 48271", "Tstart and Tstop must be >= 0.0"),
    ("all langevin/mdp 300 -5 0.1 48271", "Tstart and Tstop must be >= 0.0"),
    ("all langevin/mdp 300 300 0.1 0", "seed must be an integer > 0"),
    ("all langevin/mdp 300 300 0.1 -3", "seed must be an integer > 0"),
    ("all langevin/mdp 300 300 0.1 1.5", "seed must be an integer > 0"),
    ("all langevin/mdp 300 300 x 48271", "bad damp value x"),
    ("all langevin/mdp 300 300 0.1 48271 scale 1 0.0", "scale ratio must be > 0.0"),
    ("all langevin/mdp 300 300 0.1 48271 scale 3 2.0", "scale type 3 out of range"),
    ("all langevin/mdp 300 300 0.1 48271 scale 1", "scale needs a type and a ratio"),
    ("all langevin/mdp 300 300 0.1 48271 gjf vhalf", "keyword gjf is not supported"),
    ("all langevin/mdp 300 300 0.1 48271 angmom 1.0", "keyword angmom is not supported"),
    ("all langevin/mdp 300 300 0.1 48271 omega yes", "keyword omega is not supported"),
    ("all langevin/mdp 300 300 0.1 48271 tally maybe", "tally takes yes or no"),
    ("all langevin/mdp 300 300 0.1 48271 zero", "zero needs a value"),
    ("all langevin/mdp 300 300 0.1 48271 bogus 1", "unknown keyword bogus"),
])
def test_langevin_mdp_refusals(args, msg):
    rc, out, err = _run(LOAD + "fix 2 " + args + "\n")
    assert rc == 1
    assert msg in err, err


def test_unfix_of_an_unknown_id_is_refused():
    rc, out, err = _run(LOAD + "fix 2 all langevin/mdp 300 300 0.1 48271\nunfix 2\nunfix 2\n")
    assert rc == 1
    assert "Could not find fix ID 2 to delete" in err
