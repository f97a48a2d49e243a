"""The FIRE minimiser under random `min_modify` settings (defaults, every degenerate value, halfstepback / initialdelay
off, starting time steps of 1 - 4 fs): 80 device iterations replayed one at a time in tests/fireref.py, the forces of
every iteration against the oracle's.  usage: python3 profiles/fire_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("fire", sys.argv[1:])
