"""Randomised runs of the plugins on N ranks of the mini-host: for random MoS2 / Al-Si inputs (size, temperature, skin, run
length, seed) the thermo rows of `minilmp -np N` -- in host mode and under `fix nve/mdp` on the library's bricks; on one rank: the fix in its
default mode and with `bricks yes` -- must be the rows of the one-rank run with the host's own `fix nve` (printed digits: rel 5e-7).  usage: python3 profiles/minilmp_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("minilmp", sys.argv[1:])
