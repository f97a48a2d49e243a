"""Randomised runs of what `fix nve/mdp` does on one rank in its default mode (the C-ABI underneath: mdp_hnve_initial / compute
with f == NULL / mdp_hnve_final, the images kept by the library, the device's displacement check read one step late and a
HOST reneighboring -- download, wrap, new ghosts, re-upload of atoms and velocities -- when it fires): random MoS2 cells, random
temperatures up to 3 000 K, a projectile in some, against velocity-Verlet on the host around the ORACLE (the loop of
tests/test_gpu_trajectory.py).  usage: python3 profiles/hnve_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("hnve", sys.argv[1:])
