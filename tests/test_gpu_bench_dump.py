"""GPU: `bench.py --dump-outputs DIR` on the real path.  Two runs with the same arguments dump the same atoms with the same
values, and two rank processes (library transport, sharing this GPU through the RCCL test double of tests/native) dump
what the one-rank run dumps: the arrays are comparable from build to build and across rank counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lammps_plugins_amd.host import capi, system as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REP = (6, 6, 4)
# (thermo every step: whatever the step count, the last step tallies energy and virial)
ARGS = ["--steps", "35", "--replicate", *map(str, REP), "--temp", "300", "--thermo", "1",
        "--no-cpu-baseline", "--no-host-mode", "--no-secondary"]


def _bench(out, gpus=1, warmup=5):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    if gpus > 1:
        if not os.path.exists(capi.FAKE_RCCL):
            subprocess.run(["make", "-C", os.path.join(ROOT, "lammps-plugins_amd"), "rccl-double"], check=True)
        # a fixed order of compute against exchanges: a short policy trial, the same length in every run
        env.update(MDP_RCCL_LIBRARY=capi.FAKE_RCCL, MDP_FAKE_RCCL_TIMEOUT_S="60", MDP_OVERLAP_POLICY="split")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--warmup", str(warmup), *ARGS,
                        "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=800)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    return line, {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}


@pytest.mark.timeout(900)
def test_dump_outputs_repeat_and_agree_across_rank_counts(tmp_path):
    # the ranks' overlap-policy trial moves the atoms too (`step` counts it): the one-rank runs warm up that much longer
    l2, c = _bench(tmp_path / "two", gpus=2)
    assert l2["n_gpus"] == 2 and "TEST DOUBLE" in l2["config"]["transport"]
    step = l2["dump_outputs"]["step"]
    assert 40 <= step <= 40 + 80
    l1, a = _bench(tmp_path / "one", warmup=step - 35)
    _, b = _bench(tmp_path / "again", warmup=step - 35)
    n = 288 * int(np.prod(REP))
    assert l1["steps"] == 35 and l1["dump_outputs"]["step"] == step and l1["dump_outputs"]["atoms_dumped"] == n
    assert set(a) == {"tags", "positions", "velocities", "forces", "energy_virial"}
    assert all(v.dtype == np.float64 for v in a.values())
    np.testing.assert_array_equal(a["tags"], np.arange(1, n + 1))
    assert np.abs(a["forces"]).max() > 0.1 and np.abs(a["velocities"]).max() > 1e-3
    box = S.replicate(S.rebomos_bulk_cell(), REP).box
    for other, tol in ((b, 1e-9), (c, 1e-7)):
        np.testing.assert_array_equal(other["tags"], a["tags"])
        dx = other["positions"] - a["positions"]
        dx -= np.round(box.x2lamda(dx + box.lo)) @ box.h.T          # same atom, possibly another periodic image
        assert np.abs(dx).max() < tol
        assert np.abs(other["velocities"] - a["velocities"]).max() < tol
        assert np.abs(other["forces"] - a["forces"]).max() < 100 * tol
        np.testing.assert_allclose(other["energy_virial"], a["energy_virial"], rtol=1e-8, atol=1e-4)
