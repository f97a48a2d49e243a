"""compute rdf/mdp and compute adf/mdp on one context per rank against the brute-force references tests/rdfref.py and
tests/adfref.py: MoS2 replicas and alloys (sheared, relabelled to 3 - 12 types), 1 - 8 bricks, a free dimension, groups that
are slabs, modulus classes, 2 - 3 atoms or all but one type, 1 - 32 columns and triples, 1 - 8192 bins, cutoffs from the
first shell to cutghost - skin, MDP_MEASURE_GRID unset, 1, 3 or 64.  Integer brackets: every miscount fails.
usage: python3 profiles/measure_fuzz.py <cases> <seed>
The cases, the runs and their limits live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("measure", sys.argv[1:])
