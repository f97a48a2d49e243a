"""Randomised device-resident trajectories against the same trajectories driven on the host with ORACLE forces (the harness of
tests/test_gpu_trajectory.py): random small MoS2 cells and Al-Si alloys, random temperatures up to 4 000 K (one atom in 64
would not do here), random seeds, a fast projectile in some of them, 120 steps with the device's own deferred checks, row
prunings, list rebuilds and reneighborings.  Positions 1e-8 A (hot cases 1e-6: the trajectories are chaotic), energy 1e-9 eV
per atom.  usage: python3 profiles/trajectory_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("trajectory", sys.argv[1:])
