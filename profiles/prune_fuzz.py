"""Randomised check of the dynamic row pruning and of the pair queues (one GPU, minihost/ddhost.cpp): random hot / drifting /
strained-by-temperature runs with the kernels walking PRUNED rows (default) against the same run with MDP_PRUNE=0 (rows as
built), against MDP_LJ_QUEUE=1 / 0 (cubic-branch pairs queued / found by a second walk) and against other inner skins of the
style's own lists (MDP_INNER_SKIN: other rebuild steps, the same pairs).  The validity of pruned rows
rests on a displacement trigger read one step late with a margin: a pair missed because of it would show here as a
trajectory that leaves its twin.  usage: python3 profiles/prune_fuzz.py <cases> <seed>
The cases, the runs and their tolerances live in tests/nets.py; tests/test_gpu_nets.py runs them at fixed seeds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests")); sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (registers the package)
import nets  # noqa: E402

nets.main("prune", sys.argv[1:])
