"""The constant-flux heat sources on every one-rank path of the integrate kernel (resident with and without the device's
check, host-linked from a shuffled host order) against tests/heatref.py around the oracle: 1 - 4 sources on shuffled group
bits, a nevery per source, first steps up to 2^32 + 7, time steps of 0.5 - 2 fs, integrate group `all` or a part of the
cell, sources that are modulus classes, slabs, 2 - 3 atoms or the rest of the group, a second run from a due step.
usage: python3 profiles/heat_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("heat", sys.argv[1:])
