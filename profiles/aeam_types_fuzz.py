"""Randomised AEAM runs with 3 - 12 atom types (relabelled copies of the bundled two-element file, tests/aeam_five.py: every
new element behaves as Al or as Si, so the oracle on the relabelled file is the reference): tile kernels with per-entry
types for up to 8 types, the generic kernels beyond.  Random type counts, compositions, sizes, temperatures; 30 device-resident
steps, then forces and energy against the oracle on the final positions.  usage: python3 profiles/aeam_types_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("aeam_types", sys.argv[1:])
