"""Randomised parity at scale: random systems of 70 000 - 390 000 atoms (MoS2 replicas scaled by 0.97 - 1.12 with jitter, or
Al-Si alloys with 0 - 20 % Si) run device-resident for 20 - 60 steps from a random temperature (300 - 3 000 K; lists rebuilt
and rows pruned on the device's own triggers), then the forces of ~400-atom blocks at the box corners, the brick seams, the
last tile and random places are compared with the ORACLE's for the same atoms (tests/blockcheck.py).  1e-9 eV/A.
usage: python3 profiles/block_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("block", sys.argv[1:])
