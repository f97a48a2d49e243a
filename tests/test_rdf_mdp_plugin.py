"""CPU: `compute rdf/mdp` at the plugin boundary -- rdfmdpplugin.so exports the one C symbol `plugin load` looks up,
registers one compute style, and refuses bad input with a message naming the problem before a device is touched; the
mini-host's thermo takes c_ID[i][j] of a global array compute and refuses what is not an element of it."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load rdfmdpplugin.so\n" + HEAD


def test_rdf_plugin_exports_only_lammpsplugin_init_and_holds_the_compute():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "rdfmdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS13ComputeRDFMDP13compute_arrayEv", out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


def test_rdf_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "compute r all rdf/mdp 100\ncompute p all rdf/mdp 50 1 1 1*2 * *2 2* cutoff 4.5\n"
                        "group al type 1\ncompute g al rdf/mdp 20 * *\ncompute r all rdf/mdp 8192\n")
    assert rc == 0, err
    assert "Loaded 1 plugins from rdfmdpplugin.so" in out


@pytest.mark.parametrize("tail,msg", [
    ("compute r all rdf/mdp", "compute ID GROUP rdf/mdp Nbin"),
    ("compute r all rdf/mdp 0", "Nbin must be a whole number >= 1, not 0"),
    ("compute r all rdf/mdp ten", "Nbin must be a whole number >= 1, not ten"),
    ("compute r all rdf/mdp 50 1", "the type arguments come in pairs itype jtype, and there are 1"),
    ("compute r all rdf/mdp 50 1 1 2", "the type arguments come in pairs itype jtype, and there are 3"),
    ("compute r all rdf/mdp 50 1 3", "type 3 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute r all rdf/mdp 50 0 1", "type 0 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute r all rdf/mdp 50 2*1 1", "type 2*1 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute r all rdf/mdp 50 1 1 bogus 1", "unknown keyword bogus"),
    ("compute r all rdf/mdp 50 cutoff", "cutoff needs a value"),
    ("compute r all rdf/mdp 50 cutoff 0", "cutoff must be > 0, not 0"),
    ("compute r all rdf/mdp 50 cutoff -2.5", "cutoff must be > 0, not -2.5"),
    ("compute r all rdf/mdp 50 cutoff far", "bad cutoff value far"),
    ("compute r nobody rdf/mdp 50", "could not find compute group ID nobody"),
    ("group si type 2\ncompute r si rdf/mdp 50", "group si is empty: there is no pair to count"),
    ("compute r all rdf/mdp 50" + " 1 1" * 33, "33 type pairs; at most 32 fit one compute"),
    ("compute r all rdf/mdp 8193", "8193 bins x 1 pairs; the device's histogram holds 8192 counters"),
    ("compute r all rdf", "Unrecognized compute style 'rdf'"),
])
def test_rdf_mdp_refusals(tail, msg):
    rc, out, err = _run(LOAD + tail + "\n")
    assert rc == 1
    assert msg in err, err


@pytest.mark.parametrize("cols,msg", [
    ("c_r[51][1]", "Thermo custom compute r is an array of 50 x 5: c_r[51][1] is not one of its elements"),
    ("c_r[1][6]", "Thermo custom compute r is an array of 50 x 5: c_r[1][6] is not one of its elements"),
    ("c_r[0][1]", "Thermo custom compute r is an array of 50 x 5: c_r[0][1] is not one of its elements"),
    ("c_r[3]", "Thermo custom compute r is a vector of 0: c_r[3] is not one of its elements"),
    ("c_m[1][1]", "Thermo custom compute m is an array of 0 x 0: c_m[1][1] is not one of its elements"),
    ("c_m[5]", "Thermo custom compute m is a vector of 4: c_m[5] is not one of its elements"),
])
def test_thermo_refuses_what_is_not_an_element(cols, msg):
    rc, out, err = _run("plugin load msdmdpplugin.so\n" + LOAD + "compute r all rdf/mdp 50 1 1 1 2\ncompute m all msd/mdp\n"
                        f"thermo_style custom step {cols}\n")
    assert rc == 1
    assert msg in err, err


def test_thermo_accepts_the_elements():
    rc, out, err = _run("plugin load msdmdpplugin.so\n" + LOAD + "compute r all rdf/mdp 50 1 1 1 2\ncompute m all msd/mdp\n"
                        "thermo_style custom step c_r[1][1] c_r[50][5] c_m[4] c_later[7][7]\n")
    assert rc == 0, err
