"""compute profile/mdp, msd/mdp and heatflux/mdp on one context per rank against tests/profileref.py, tests/msdref.py and
tests/heatfluxref.py on the state gathered by tag from the same run, the last heat current also against the oracle: MoS2
replicas and alloys (all three tilts in some), 0 - 2 500 K, drifts up to 150 A/ps, 1 - 8 bricks, a free dimension, groups that
are slabs, modulus classes, all but one type, 1 - 3 atoms or nobody on bit 1, 7, 30 or 31, profile grids of 1 - 3 dimensions
from 1 row to PROFILE_MAXBINS with 819 and 820 rows among them, MDP_MEASURE_GRID unset, 1, 3 or 64, msd origins from the
current positions or by tag, at the start or mid-run, a last half left to the first read.
usage: python3 profiles/peratom_fuzz.py <cases> <seed>
The cases, the runs and their limits live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("peratom", sys.argv[1:])
