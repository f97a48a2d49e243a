"""compute coord/atom/mdp, centro/atom/mdp and cna/atom/mdp, all three on one context per rank, against tests/structref.py and
tests/cnaref.py on positions gathered by tag from the same state: MoS2 replicas and alloys (all three tilts in some, 3 - 12 types
in some), 0 - 2 500 K, 1 - 8 bricks, a free dimension, or a constructed cell (the close-packed stack, bcc, the icosahedron);
groups that are slabs, modulus classes, all but one type, 1 - 3 atoms or nobody on bit 1, 7, 30 or 31; 1 - 32 columns, N of
2 - 64, cutoffs from just above the first shell to the radius that holds 100 atoms; MDP_MEASURE_GRID unset, 1, 3 or 64; and
after the last read a second parameter set on the same contexts, or the first set up afresh.
usage: python3 profiles/structure_fuzz.py <cases> <seed>
The cases, the runs and their limits live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("structure", sys.argv[1:])
