"""The two post-force stages -- fix indent/mdp and fix spring/mdp -- on every one-rank path of the integrate kernel (resident
with and without the device's check; host-linked from a shuffled host order, indenters alone) against tests/springref.py
and tests/indentref.py around the oracle: 0 - 4 indenters of every shape, side and dim on shuffled group bits, 0 - 4
springs with every `use`, sheared cells, a free dimension, centres a box vector away, r == 0, a second run, a new mask.
usage: python3 profiles/postforce_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("postforce", sys.argv[1:])
