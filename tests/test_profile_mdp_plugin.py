"""CPU: `compute profile/mdp` at the plugin boundary -- profilemdpplugin.so exports the one C symbol `plugin load` looks up,
registers one compute style, and refuses bad input with a message naming the problem before a device is touched."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load profilemdpplugin.so\n" + HEAD


def test_profile_plugin_exports_only_lammpsplugin_init_and_holds_the_compute():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "profilemdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS17ComputeProfileMDP13compute_arrayEv", out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


def test_profile_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "compute p all profile/mdp x 7 com yes\ncompute q all profile/mdp x 3 z 4\n"
                        "compute r all profile/mdp z 16 y 16 x 16 com no\ngroup al type 1\ncompute g al profile/mdp com yes y 200\n"
                        "compute big all profile/mdp x 1024 y 1024\n"
                        "thermo_style custom step c_p[7][8] c_q[12][9] c_r[4096][10] c_g[200][1]\n")
    assert rc == 0, err
    assert "Loaded 1 plugins from profilemdpplugin.so" in out


@pytest.mark.parametrize("tail,msg", [
    ("compute p all profile/mdp", "no dimension: compute ID GROUP profile/mdp dim N"),
    ("compute p all profile/mdp com yes", "no dimension: compute ID GROUP profile/mdp dim N"),
    ("compute p all profile/mdp x 7 x 3", "dimension x is named twice"),
    ("compute p all profile/mdp z 7 y 2 z 3", "dimension z is named twice"),
    ("compute p all profile/mdp x", "dimension x needs a number of bins"),
    ("compute p all profile/mdp x 0", "N must be a whole number >= 1, not 0"),
    ("compute p all profile/mdp x -3", "N must be a whole number >= 1, not -3"),
    ("compute p all profile/mdp x 2.5", "N must be a whole number >= 1, not 2.5"),
    ("compute p all profile/mdp x seven", "N must be a whole number >= 1, not seven"),
    ("compute p all profile/mdp x 1024 y 1025", "more than 1048576 rows"),
    ("compute p all profile/mdp x 1048577", "more than 1048576 rows"),
    ("compute p all profile/mdp x 4096 y 4096 z 4096", "more than 1048576 rows"),
    ("compute p all profile/mdp x 7 bound 0 1", "unknown keyword bound"),
    ("compute p all profile/mdp w 7", "unknown keyword w"),
    ("compute p all profile/mdp x 7 com", "com needs a value"),
    ("compute p all profile/mdp x 7 com maybe", "com takes yes or no, not maybe"),
    ("compute p nobody profile/mdp x 7", "could not find compute group ID nobody"),
    ("group si type 2\ncompute p si profile/mdp x 7", "group si is empty: there is no atom to bin"),
    ("compute p all profile/mdp x 7\nthermo_style custom step c_p[8][1]", "compute p is an array of 7 x 8: c_p[8][1] is not one of its elements"),
    ("compute p all profile/mdp x 3 z 4\nthermo_style custom step c_p[1][10]", "compute p is an array of 12 x 9: c_p[1][10] is not one of its elements"),
    ("compute p all profile", "Unrecognized compute style 'profile'"),
])
def test_profile_mdp_refusals(tail, msg):
    rc, out, err = _run(LOAD + tail + "\n")
    assert rc == 1
    assert msg in err, err
