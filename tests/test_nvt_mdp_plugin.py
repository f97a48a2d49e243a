"""CPU: `fix nvt/mdp` at the plugin boundary -- nvtmdpplugin.so exports the one C symbol `plugin load` looks up, registers
one style, and refuses bad input with a message naming the problem before a device is touched."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import PKG, _run

LOAD = "plugin load nvtmdpplugin.so\n"


def test_nvt_plugin_exports_only_lammpsplugin_init_and_holds_the_fix():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "nvtmdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS9FixNVTMDP14compute_scalarEv", out)


def test_nvt_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "fix 1 all nvt/mdp temp 300.0 300.0 0.1\n")
    assert rc == 0, err
    assert "Loaded 1 plugins from nvtmdpplugin.so" in out


@pytest.mark.parametrize("args,msg", [
    ("mobile nvt/mdp temp 300 300 0.1", "requires group all"),
    ("all nvt/mdp tchain 3", "requires the temp keyword"),
    ("all nvt/mdp temp 300 300 0.0", "Tdamp must be > 0.0"),
    ("all nvt/mdp temp 0.0 300 0.1", "Tstart and Tstop must be > 0.0"),
    ("all nvt/mdp temp 300 -5 0.1", "Tstart and Tstop must be > 0.0"),
    ("all nvt/mdp temp 300 300 0.1 tchain 0", "tchain must be >= 1"),
    ("all nvt/mdp temp 300 300 0.1 tloop 0", "tloop must be >= 1"),
    ("all nvt/mdp temp 300 300 0.1 iso 1.0 1.0 1.0", "barostat keyword iso"),
    ("all nvt/mdp temp 300 300 0.1 aniso 1.0 1.0 1.0", "barostat keyword aniso"),
    ("all nvt/mdp temp 300 300 0.1 x 1.0 1.0 1.0", "barostat keyword x"),
    ("all nvt/mdp temp 300 300 0.1 couple xyz", "barostat keyword couple"),
    ("all nvt/mdp temp 300 300 0.1 mtk yes", "barostat keyword mtk"),
    ("all nvt/mdp temp 300 300 0.1 dilate all", "barostat keyword dilate"),
    ("all nvt/mdp temp 300 300 0.1 ptemp 300", "barostat keyword ptemp"),
    ("all nvt/mdp temp 300 300 0.1 tchain", "tchain needs a value"),
    ("all nvt/mdp temp 300 300", "temp needs Tstart Tstop Tdamp"),
    ("all nvt/mdp temp 300 300 0.1 bogus 1", "unknown keyword bogus"),
])
def test_nvt_mdp_refusals(args, msg):
    rc, out, err = _run(LOAD + "fix 1 " + args + "\n")
    assert rc == 1
    assert msg in err, err
