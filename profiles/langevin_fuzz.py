"""The Langevin thermostat on every path of the integrate kernel (resident with and without the device's check,
host-linked, 2 - 8 bricks with migrating atoms) against velocity Verlet + tests/langevinref.py around the oracle: first
steps across 2^32, time steps of 0.5 - 2 fs, ramps up and down to 0 K, ratios, zero, tally, sheared boxes.
usage: python3 profiles/langevin_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("langevin", sys.argv[1:])
