"""CPU: `compute cna/atom/mdp` at the plugin boundary -- the plugin file exports the one C symbol `plugin load` looks up, registers
one compute style, and refuses bad input with a message naming the problem before a device is touched; the mini-host takes the
compute as a per-atom vector (dump custom, compute reduce) and as a global vector of 5 (thermo c_ID[k]).  The refusals that
need a run to be seen (the host-linked mode, no pair style, Rc beyond cutforce) are in tests/test_gpu_cna_mdp_plugin.py."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load cnamdpplugin.so\n" + HEAD
ONE = LOAD + "compute s all cna/atom/mdp 3.45\n"


def test_the_plugin_exports_only_lammpsplugin_init_and_holds_the_compute():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "cnamdpplugin.so")], capture_output=True, text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    for method in ("15compute_peratomEv", "14compute_vectorEv"):
        assert re.search(r"_ZN9LAMMPS_NS17ComputeCnaAtomMDP" + method, out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


def test_the_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "compute a all cna/atom/mdp 3.4528\ncompute b all cna/atom/mdp 1e-1\ngroup al type 1\n"
                               "compute c al cna/atom/mdp 3.986\ncompute d all cna/atom/mdp 25\n")     # (Rc against cutforce: at init)
    assert rc == 0, err
    assert "Loaded 1 plugins from cnamdpplugin.so" in out


@pytest.mark.parametrize("tail,msg", [
    ("compute a all cna/atom/mdp", "Illegal compute cna/atom/mdp command: compute ID GROUP cna/atom/mdp Rc"),
    ("compute a all cna/atom/mdp 3.5x", "bad Rc value 3.5x"),
    ("compute a all cna/atom/mdp fcc", "bad Rc value fcc"),
    ("compute a all cna/atom/mdp inf", "bad Rc value inf"),
    ("compute a all cna/atom/mdp nan", "bad Rc value nan"),
    ("compute a all cna/atom/mdp 0", "Rc must be > 0, not 0"),
    ("compute a all cna/atom/mdp -3.45", "Rc must be > 0, not -3.45"),
    ("compute a all cna/atom/mdp 3.45 3.45", "nothing follows Rc, not 3.45: compute ID GROUP cna/atom/mdp Rc"),
    ("compute a all cna/atom/mdp 3.45 cutoff 3.45", "nothing follows Rc, not cutoff"),
    ("compute a nobody cna/atom/mdp 3.45", "could not find compute group ID nobody"),
    ("group si type 2\ncompute a si cna/atom/mdp 3.45", "group si is empty: there is no atom to look around"),
    ("compute a all cna/atom 3.45", "Unrecognized compute style 'cna/atom'"),
])
def test_refusals_before_any_device(tail, msg):
    rc, out, err = _run(LOAD + tail + "\n")
    assert rc == 1
    assert msg in err, err


@pytest.mark.parametrize("tail,msg", [
    ("dump d all custom 10 f.dump id c_s[1]", "Dump custom compute s does not calculate a per-atom array"),
    ("compute r all reduce max c_s[2]", "Compute reduce compute s does not calculate a per-atom array"),
    ("thermo_style custom step c_s[0]", "Thermo custom compute s is a vector of 5: c_s[0] is not one of its elements"),
    ("thermo_style custom step c_s[6]", "Thermo custom compute s is a vector of 5: c_s[6] is not one of its elements"),
    ("thermo_style custom step c_s[1][1]", "c_s[1][1] is not one of its elements"),
])
def test_the_mini_host_refuses(tail, msg):
    rc, out, err = _run(ONE + tail + "\n")
    assert rc == 1
    assert msg in err, err


def test_the_mini_host_accepts_both_faces():
    """the per-atom vector in a dump and under compute reduce, the census in the thermo, all of one compute"""
    rc, out, err = _run(ONE + "dump d all custom 10 a.*.dump id type x y z c_s\ncompute r all reduce max c_s\ncompute m all reduce min c_s\n"
                              "thermo_style custom step c_s[1] c_s[2] c_s[3] c_s[4] c_s[5] c_r c_m\n")
    assert rc == 0, err
