"""Randomised force parity: random MoS2 cells (scale 0.92-1.16, jitter up to 0.25 A, small replicas) and random Al-Si alloys
(4-7 fcc cells, 0-50 % Si, jitter up to 0.3 A) through the HIP path (host mode, device-built lists, every tally on, then a
force-only call) against a LIVE oracle compute on the same inputs.  Tolerances of tests/test_gpu_golden.py.
usage: python3 profiles/force_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("force", sys.argv[1:])
