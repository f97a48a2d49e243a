"""CPU: `compute coord/atom/mdp` and `compute centro/atom/mdp` at the plugin boundary -- each plugin file exports the one C symbol
`plugin load` looks up, registers one compute style, and refuses bad input with a message naming the problem before a device
is touched; the mini-host's `dump custom` with a c_ column, its built-in `compute reduce` and its thermo refuse what is no
per-atom (or no global) value, and a dump without c_ columns still does nothing."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load coordmdpplugin.so\nplugin load centromdpplugin.so\n" + HEAD
BOTH = LOAD + "compute c all coord/atom/mdp cutoff 3.5\ncompute t all coord/atom/mdp cutoff 3.5 1 2 *\ncompute s all centro/atom/mdp fcc\n"


@pytest.mark.parametrize("so,cls", [("coordmdpplugin.so", "ComputeCoordAtomMDP"), ("centromdpplugin.so", "ComputeCentroAtomMDP")])
def test_the_plugin_exports_only_lammpsplugin_init_and_holds_the_compute(so, cls):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, so)], capture_output=True, text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS%d%s15compute_peratomEv" % (len(cls), cls), out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


@pytest.mark.parametrize("so,lines", [
    ("coordmdpplugin.so", "compute a all coord/atom/mdp cutoff 3.5\ncompute b all coord/atom/mdp cutoff 2.8 2\n"
                          "compute c all coord/atom/mdp cutoff 6.5 1 2 * 1* *2 1*2\ngroup al type 1\ncompute d al coord/atom/mdp cutoff 1e-1 *\n"
                          "compute e all coord/atom/mdp cutoff 3.5" + " 1" * 32 + "\n"),
    ("centromdpplugin.so", "compute a all centro/atom/mdp fcc\ncompute b all centro/atom/mdp bcc cutoff 3.5\ncompute c all centro/atom/mdp 2\n"
                           "compute d all centro/atom/mdp 64 cutoff 6.5\ngroup al type 1\ncompute e al centro/atom/mdp 6 cutoff 4.0\n"),
])
def test_the_plugin_registers_one_style(so, lines):
    rc, out, err = _run(f"plugin load {so}\n" + HEAD + lines)
    assert rc == 0, err
    assert f"Loaded 1 plugins from {so}" in out


@pytest.mark.parametrize("tail,msg", [
    ("compute a all coord/atom/mdp", "compute ID GROUP coord/atom/mdp cutoff Rc [jtype ...]"),
    ("compute a all coord/atom/mdp cutoff", "compute ID GROUP coord/atom/mdp cutoff Rc [jtype ...]"),
    ("compute a all coord/atom/mdp 3.5", "compute ID GROUP coord/atom/mdp cutoff Rc [jtype ...]"),
    ("compute a all coord/atom/mdp cutoff 3.5x", "bad Rc value 3.5x"),
    ("compute a all coord/atom/mdp cutoff inf", "bad Rc value inf"),
    ("compute a all coord/atom/mdp cutoff 0", "Rc must be > 0, not 0"),
    ("compute a all coord/atom/mdp cutoff -2.8", "Rc must be > 0, not -2.8"),
    ("compute a all coord/atom/mdp cutoff 3.5 3", "type 3 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute a all coord/atom/mdp cutoff 3.5 1 0", "type 0 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute a all coord/atom/mdp cutoff 3.5 2*1", "type 2*1 is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute a all coord/atom/mdp cutoff 3.5 one", "type one is not N, *, N*, *M or N*M within 1 .. 2"),
    ("compute a all coord/atom/mdp cutoff 3.5" + " 1" * 33, "33 columns; at most 32 fit one compute"),
    ("compute a all coord/atom/mdp orientorder o 0.5", "the orientorder form is not supported"),
    ("compute a all coord/atom/mdp cutoff 3.5 group all", "the group keyword is not supported: the partners of a centre are the atoms of every group"),
    ("compute a all coord/atom/mdp cutoff 3.5 1 group all", "the group keyword is not supported"),
    ("compute a nobody coord/atom/mdp cutoff 3.5", "could not find compute group ID nobody"),
    ("group si type 2\ncompute a si coord/atom/mdp cutoff 3.5", "group si is empty: there is no atom to count around"),
    ("compute a all coord/atom cutoff 3.5", "Unrecognized compute style 'coord/atom'"),
    ("compute a all centro/atom/mdp", "compute ID GROUP centro/atom/mdp fcc|bcc|N [cutoff Rc]"),
    ("compute a all centro/atom/mdp hcp", "the lattice is fcc, bcc or a whole number N of neighbours, not hcp"),
    ("compute a all centro/atom/mdp 12.0", "the lattice is fcc, bcc or a whole number N of neighbours, not 12.0"),
    ("compute a all centro/atom/mdp 7", "N must be an even whole number >= 2, not 7"),
    ("compute a all centro/atom/mdp 0", "N must be an even whole number >= 2, not 0"),
    ("compute a all centro/atom/mdp -2", "N must be an even whole number >= 2, not -2"),
    ("compute a all centro/atom/mdp 66", "N = 66; at most 64 neighbours fit the device's list of pair values"),
    ("compute a all centro/atom/mdp 200", "N = 200; at most 64 neighbours fit"),
    ("compute a all centro/atom/mdp fcc axes yes", "the axes keyword is not supported"),
    ("compute a all centro/atom/mdp fcc cutoff", "cutoff needs a value"),
    ("compute a all centro/atom/mdp fcc cutoff 0", "Rc must be > 0, not 0"),
    ("compute a all centro/atom/mdp fcc cutoff x", "bad Rc value x"),
    ("compute a all centro/atom/mdp fcc radius 3", "unknown keyword radius"),
    ("compute a nobody centro/atom/mdp fcc", "could not find compute group ID nobody"),
    ("group si type 2\ncompute a si centro/atom/mdp fcc", "group si is empty: there is no atom to look around"),
    ("compute a all centro/atom fcc", "Unrecognized compute style 'centro/atom'"),
])
def test_refusals_before_any_device(tail, msg):
    rc, out, err = _run(LOAD + tail + "\n")
    assert rc == 1
    assert msg in err, err


@pytest.mark.parametrize("tail,msg", [
    ("dump d all custom 10 f.dump id c_x", "Could not find Dump custom compute ID: x"),
    ("compute r all reduce max c_s\ndump d all custom 10 f.dump id c_r", "Dump custom compute r does not compute per-atom info"),
    ("dump d all custom 10 f.dump id c_t", "Dump custom compute t does not calculate a per-atom vector: it has 3 columns"),
    ("dump d all custom 10 f.dump id c_t[4]", "Dump custom compute t has 3 columns: c_t[4] is accessed out-of-range"),
    ("dump d all custom 10 f.dump id c_t[0]", "Dump custom compute t has 3 columns: c_t[0] is accessed out-of-range"),
    ("dump d all custom 10 f.dump id c_c[1]", "Dump custom compute c does not calculate a per-atom array"),
    ("dump d all custom 10 f.dump id vx c_c", "not the column vx"),
    ("dump d all custom 0 f.dump id c_c", "N must be a whole number >= 1, not 0"),
    ("dump d nobody custom 10 f.dump id c_c", "Could not find dump group ID nobody"),
    ("dump d all atom 10 f.dump id c_c", "minilmp supports `dump ID GROUP custom N FILE id type x y z c_ID c_ID[k] ...` only"),
    ("dump d all custom 10 f.dump id c_c\ndump d all custom 10 g.dump id c_s", "Reuse of dump ID 'd'"),
    ("compute r all reduce max c_x", "Could not find Compute reduce compute ID: x"),
    ("compute r all reduce max c_s\ncompute q all reduce sum c_r", "Compute reduce compute r does not compute per-atom info"),
    ("compute r all reduce median c_s", "the mode is sum, ave, min or max, not median"),
    ("compute r all reduce max c_t", "Compute reduce compute t does not calculate a per-atom vector"),
    ("compute r all reduce max c_t[4]", "c_t[4] is accessed out-of-range"),
    ("compute r all reduce max c_s c_c", "minilmp supports `compute ID GROUP reduce sum|ave|min|max c_ID|c_ID[k]` over one per-atom compute only"),
    ("compute r all reduce max v_x", "not the input v_x"),
    ("compute r nobody reduce max c_s", "Could not find compute group ID nobody"),
    ("thermo_style custom step c_s", "Thermo custom compute s computes per-atom values: c_s is no global value"),
    ("thermo_style custom step c_c[1]", "Thermo custom compute c computes per-atom values"),
    ("thermo_style custom step c_t[1][2]", "Thermo custom compute t computes per-atom values"),
    ("compute r all reduce max c_s\nthermo_style custom step c_r[1]", "Thermo custom compute r is a vector of 0"),
])
def test_the_mini_host_refuses(tail, msg):
    rc, out, err = _run(BOTH + tail + "\n")
    assert rc == 1
    assert msg in err, err


def test_the_mini_host_accepts(tmp_path):
    """per-atom columns of both kinds in a dump, reductions of both, the reductions in the thermo; and a dump without c_ columns --
    of a style the host never writes, with columns it does not know -- is accepted and ignored as ever, and no file appears"""
    ghost = tmp_path / "never.dump"
    rc, out, err = _run(BOTH + "dump d all custom 10 a.*.dump id type x y z c_c c_t[1] c_t[3] c_s\n"
                        "compute r all reduce max c_s\ncompute m all reduce min c_t[2]\ncompute a all reduce ave c_c\ncompute u all reduce sum c_c\n"
                        "thermo_style custom step c_r c_m c_a c_u\n"
                        f"dump e all custom 10 {ghost} id x y z vx vy vz fx\ndump f all atom 5 {ghost}\ndump g all xyz 1 {ghost}\n"
                        "dump_modify e sort id\n")
    assert rc == 0, err
    assert not ghost.exists()
