"""CPU: `compute adf/mdp` at the plugin boundary -- adfmdpplugin.so exports the one C symbol `plugin load` looks up,
registers one compute style, and refuses bad input with a message naming the problem before a device is touched; the
mini-host's thermo takes the elements of its Nbin x (1 + 2 Ntriple) array and refuses what is not one."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load adfmdpplugin.so\n" + HEAD
FIRST = " 0 3.5 0 3.5"


def test_adf_plugin_exports_only_lammpsplugin_init_and_holds_the_compute():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "adfmdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS13ComputeADFMDP13compute_arrayEv", out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


def test_adf_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "compute a all adf/mdp 90\n"
                        f"compute p all adf/mdp 45 1 1 1{FIRST} 1*2 * *2 0 3.5 3.5 4.5 2* *1 1*1 .5 3.5 1e-1 4 ordinate cosine cumulative centre\n"
                        "compute q all adf/mdp 45 cumulative fraction ordinate radian\ncompute d all adf/mdp 45 ordinate degree\n"
                        f"group al type 1\ncompute g al adf/mdp 20 * * *{FIRST}\ncompute a all adf/mdp 8192\n")
    assert rc == 0, err
    assert "Loaded 1 plugins from adfmdpplugin.so" in out


@pytest.mark.parametrize("tail,msg", [
    ("compute a all adf/mdp", "compute ID GROUP adf/mdp Nbin [itype jtype ktype Rjinner Rjouter Rkinner Rkouter ...]"),
    ("compute a all adf/mdp 0", "Nbin must be a whole number >= 1, not 0"),
    ("compute a all adf/mdp ten", "Nbin must be a whole number >= 1, not ten"),
    ("compute a all adf/mdp 4.5", "Nbin must be a whole number >= 1, not 4.5"),
    ("compute a all adf/mdp 45 1 1 1", "the triple arguments come in sevens itype jtype ktype Rjinner Rjouter Rkinner Rkouter, and there are 3"),
    ("compute a all adf/mdp 45 1 1 1 0 3.5 0", "come in sevens itype jtype ktype Rjinner Rjouter Rkinner Rkouter, and there are 6"),
    (f"compute a all adf/mdp 45 1 1 1{FIRST} 2", "come in sevens itype jtype ktype Rjinner Rjouter Rkinner Rkouter, and there are 8"),
    (f"compute a all adf/mdp 45 1 3 1{FIRST}", "type 3 is not N, *, N*, *M or N*M within 1 .. 2"),
    (f"compute a all adf/mdp 45 0 1 1{FIRST}", "type 0 is not N, *, N*, *M or N*M within 1 .. 2"),
    (f"compute a all adf/mdp 45 1 1 2*1{FIRST}", "type 2*1 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute a all adf/mdp 45 1 1 1 0 3.5x 0 3.5", "bad radius value 3.5x"),
    ("compute a all adf/mdp 45 1 1 1 0 3.5 0 +inf", "bad radius value +inf"),
    ("compute a all adf/mdp 45 1 1 1 -1 3.5 0 3.5", "a radius must be >= 0, not -1"),
    ("compute a all adf/mdp 45 1 1 1 3.5 3.5 0 3.5", "triple 1: the inner radius 3.5 is not below the outer radius 3.5"),
    (f"compute a all adf/mdp 45 1 1 1{FIRST} 1 1 1 0 3.5 4 3", "triple 2: the inner radius 4 is not below the outer radius 3"),
    ("compute a all adf/mdp 45" + (" 1 1 1" + FIRST) * 33, "33 triples; at most 32 fit one compute"),
    ("compute a all adf/mdp 8193", "8193 bins x 1 triples; the device's histogram holds 8192 counters"),
    ("compute a all adf/mdp 4097" + (" 1 1 1" + FIRST) * 2, "4097 bins x 2 triples; the device's histogram holds 8192 counters"),
    (f"compute a all adf/mdp 45 1 1 1{FIRST} bogus 1", "unknown keyword bogus"),
    ("compute a all adf/mdp 45 cutoff 3.5", "unknown keyword cutoff"),
    ("compute a all adf/mdp 45 ordinate", "ordinate needs a value"),
    ("compute a all adf/mdp 45 ordinate grad", "ordinate takes degree, radian or cosine, not grad"),
    ("compute a all adf/mdp 45 cumulative", "cumulative needs a value"),
    ("compute a all adf/mdp 45 cumulative center", "cumulative takes fraction or centre, not center"),
    ("compute a nobody adf/mdp 45", "could not find compute group ID nobody"),
    ("group si type 2\ncompute a si adf/mdp 45", "group si is empty: there is no angle to count"),
    ("compute a all adf", "Unrecognized compute style 'adf'"),
])
def test_adf_mdp_refusals(tail, msg):
    rc, out, err = _run(LOAD + tail + "\n")
    assert rc == 1
    assert msg in err, err


@pytest.mark.parametrize("cols,msg", [
    ("c_a[46][1]", "Thermo custom compute a is an array of 45 x 5: c_a[46][1] is not one of its elements"),
    ("c_a[1][6]", "Thermo custom compute a is an array of 45 x 5: c_a[1][6] is not one of its elements"),
    ("c_a[0][1]", "Thermo custom compute a is an array of 45 x 5: c_a[0][1] is not one of its elements"),
    ("c_a[3]", "Thermo custom compute a is a vector of 0: c_a[3] is not one of its elements"),
    ("c_d[1][4]", "Thermo custom compute d is an array of 10 x 3: c_d[1][4] is not one of its elements"),
])
def test_thermo_refuses_what_is_not_an_element(cols, msg):
    rc, out, err = _run(LOAD + f"compute a all adf/mdp 45 1 1 1{FIRST} 2 1 1{FIRST}\ncompute d all adf/mdp 10\n"
                        f"thermo_style custom step {cols}\n")
    assert rc == 1
    assert msg in err, err


def test_thermo_accepts_the_elements():
    rc, out, err = _run(LOAD + f"compute a all adf/mdp 45 1 1 1{FIRST} 2 1 1{FIRST}\ncompute d all adf/mdp 10\n"
                        "thermo_style custom step c_a[1][1] c_a[45][5] c_d[10][3]\n")
    assert rc == 0, err
