"""Randomised multi-rank consistency runs of the C++ resident host (minihost/ddhost.cpp) on one GPU through the RCCL test
double: for random styles, rank counts, sizes, temperatures, drifts and seeds the N-rank run must end where the one-rank
run ends (positions 1e-8 A, velocities 1e-7 A/ps).  usage: python3 profiles/dd_fuzz.py <cases> <seed> [style]
(The scan bug of DESIGN section 6 showed on one configuration in dozens: this is the net for its kind.)
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("dd", sys.argv[1:])
