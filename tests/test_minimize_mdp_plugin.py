"""CPU: `minimize/mdp` at the plugin boundary -- minimizemdpplugin.so exports the one C symbol `plugin load` looks up,
registers one command style, and refuses bad input with a message naming the problem before a device is touched."""
import os
import re
import subprocess

import pytest

from test_plugin_boundary import HEAD, PKG, _run

LOAD = "plugin load minimizemdpplugin.so\n" + HEAD


def test_minimize_plugin_exports_only_lammpsplugin_init_and_holds_the_command():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "minimizemdpplugin.so")], capture_output=True,
                         text=True).stdout
    c_syms = [l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z")
              and l.split()[-1] not in ("_init", "_fini")]
    assert c_syms == ["lammpsplugin_init"]
    assert re.search(r"_ZN9LAMMPS_NS11MinimizeMDP7commandEiPPc", out)
    assert not re.search(r"FixNVEMDP", out)          # (the brick hand-over is shared as a header, the fix is not linked in)


def test_minimize_plugin_registers_one_style_and_the_word_is_unknown_without_it():
    rc, out, err = _run(LOAD)
    assert rc == 0, err
    assert "Loaded 1 plugins from minimizemdpplugin.so" in out
    rc, out, err = _run(HEAD + "minimize/mdp 0.0 1.0e-6 100 1000\n")
    assert rc == 1 and "Unknown command: minimize/mdp" in err
    # pair and fix registration are what they were: the other plugin files still count their own styles
    rc, out, err = _run("plugin load langevinmdpplugin.so\n" + LOAD)
    assert rc == 0 and "Loaded 1 plugins from langevinmdpplugin.so" in out and "Loaded 1 plugins from minimizemdpplugin.so" in out


@pytest.mark.parametrize("args,msg", [
    ("0.0 1.0e-6 100", "Illegal minimize/mdp command"),
    ("", "Illegal minimize/mdp command"),
    ("-1.0 1.0e-6 100 1000", "etol and ftol must be >= 0.0"),
    ("0.0 -1.0e-6 100 1000", "etol and ftol must be >= 0.0"),
    ("0.0 1.0e-6 -100 1000", "maxiter and maxeval must be >= 0"),
    ("0.0 1.0e-6 100 -1", "maxiter and maxeval must be >= 0"),
    ("0.0 x 100 1000", "etol and ftol must be numbers"),
    ("0.0 1.0e-6 1.5 1000", "maxiter and maxeval must be integers"),
    ("0.0 1.0e-6 100 1000 bogus 1", "unknown keyword bogus"),
    ("0.0 1.0e-6 100 1000 dmax", "dmax needs a value"),
    ("0.0 1.0e-6 100 1000 dmax 0.0", "dmax must be > 0.0"),
    ("0.0 1.0e-6 100 1000 dmax x", "bad dmax value x"),
    ("0.0 1.0e-6 100 1000 tmax 0.5", "tmax must be >= 1.0"),
    ("0.0 1.0e-6 100 1000 tmin 0.0", "tmin must be > 0.0 and <= 1.0"),
    ("0.0 1.0e-6 100 1000 tmin 2.0", "tmin must be > 0.0 and <= 1.0"),
    ("0.0 1.0e-6 100 1000 delaystep -1", "delaystep must be an integer >= 0"),
    ("0.0 1.0e-6 100 1000 delaystep 2.5", "delaystep must be an integer >= 0"),
    ("0.0 1.0e-6 100 1000 dtgrow 0.9", "dtgrow must be >= 1.0"),
    ("0.0 1.0e-6 100 1000 dtshrink 1.5", "dtshrink must be > 0.0 and <= 1.0"),
    ("0.0 1.0e-6 100 1000 dtshrink 0.0", "dtshrink must be > 0.0 and <= 1.0"),
    ("0.0 1.0e-6 100 1000 alpha0 1.0", "alpha0 must be > 0.0 and < 1.0"),
    ("0.0 1.0e-6 100 1000 alpha0 0.0", "alpha0 must be > 0.0 and < 1.0"),
    ("0.0 1.0e-6 100 1000 alphashrink 1.5", "alphashrink must be > 0.0 and <= 1.0"),
    ("0.0 1.0e-6 100 1000 halfstepback maybe", "halfstepback takes yes or no"),
    ("0.0 1.0e-6 100 1000 initialdelay 1", "initialdelay takes yes or no"),
    ("0.0 1.0e-6 100 1000 integrator verlet", "keyword integrator is not supported"),
    ("0.0 1.0e-6 100 1000 norm max", "keyword norm is not supported"),
    ("0.0 1.0e-6 100 1000 line quadratic", "keyword line is not supported"),
    ("0.0 1.0e-6 100 1000", "requires a pair style of this plugin"),       # (no pair style at all)
])
def test_minimize_mdp_refusals(args, msg):
    rc, out, err = _run(LOAD + "minimize/mdp " + args + "\n")
    assert rc == 1
    assert msg in err, err


def test_more_than_one_rank_and_a_box_that_is_not_periodic_are_refused():
    rc, out, err = _run(LOAD + "minimize/mdp 0.0 1.0e-6 100 1000\n", np=2)
    assert rc == 1 and "minimize/mdp runs on one MPI rank" in err, err
    rc, out, err = _run("boundary p p f\n" + LOAD + "minimize/mdp 0.0 1.0e-6 100 1000\n")
    assert rc == 1 and "minimize/mdp needs a periodic box" in err, err
    rc, out, err = _run("boundary p p p\n" + LOAD + "minimize/mdp 0.0 1.0e-6 100 1000\n")
    assert rc == 1 and "requires a pair style of this plugin" in err, err
