"""Randomised HOST-MODE walks (the plain plugin path: atoms uploaded once, then positions every step -- mdp_set_positions_host
-- with the library deciding by itself when its own lists and its pruned rows are stale): random cells, then 40 steps of a
random walk (every atom a little, one atom a lot, some steps nobody) inside the host's skin, forces against the oracle at
EVERY step.  usage: python3 profiles/hostmode_walk_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("hostmode_walk", sys.argv[1:])
