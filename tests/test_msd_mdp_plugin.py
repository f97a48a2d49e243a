"""CPU: `compute msd/mdp` at the plugin boundary -- msdmdpplugin.so exports the one C symbol `plugin load` looks up,
registers one compute style in the mini-host's fourth registry, and refuses bad input with a message naming the problem
before a device is touched; the mini-host keeps atom->image and writes it on request."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load msdmdpplugin.so\n" + HEAD


def test_msd_plugin_exports_only_lammpsplugin_init_and_holds_the_compute():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "msdmdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS13ComputeMSDMDP14compute_vectorEv", out)
    assert not re.search(r"FixNVEMDP", out)          # (fix nve/mdp is reached through Fix::extract, not linked in)


def test_msd_plugin_registers_one_style():
    rc, out, err = _run(LOAD + "compute m all msd/mdp\ncompute c all msd/mdp com yes average no\ncompute m all msd/mdp com no\n")
    assert rc == 0, err
    assert "Loaded 1 plugins from msdmdpplugin.so" in out


@pytest.mark.parametrize("tail,msg", [
    ("compute m all msd/mdp average yes", "average yes is not supported"),
    ("compute m all msd/mdp com yes average yes", "average yes is not supported"),
    ("compute m all msd/mdp bogus 1", "unknown keyword bogus"),
    ("compute m all msd/mdp com", "com needs a value"),
    ("compute m all msd/mdp com maybe", "com takes yes or no, not maybe"),
    ("compute m nobody msd/mdp", "could not find compute group ID nobody"),
    ("group si type 2\ncompute m si msd/mdp", "group si is empty: there is no atom to measure"),
    ("compute m all msd", "Unrecognized compute style 'msd'"),
])
def test_msd_mdp_refusals(tail, msg):
    rc, out, err = _run(LOAD + tail + "\n")
    assert rc == 1
    assert msg in err, err


def test_the_minihost_writes_the_image_flags_on_request(tmp_path):
    dump = tmp_path / "d"
    rc, out, err = _run(LOAD + f"write_dump all custom {dump} id x y z vx vy vz ix iy iz\n")
    assert rc == 0, err
    lines = dump.read_text().splitlines()
    assert lines[4] == "ITEM: ATOMS id x y z vx vy vz ix iy iz"
    rows = [l.split() for l in lines[5:]]
    assert len(rows) == 32 and all(len(r) == 10 and r[7:] == ["0", "0", "0"] for r in rows)
    rc, out, err = _run(LOAD + f"write_dump all custom {dump} id x y z ix iy iz\n")
    assert rc == 1 and "the same with `ix iy iz` behind it" in err
