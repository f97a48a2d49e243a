"""GPU: a plain `bench.py` run is the headline alone -- set-up, warm-up, the timed steps, one line.  Per-kernel times and
the roofline, the forced reneighboring, host mode, the CPU baseline and the `secondary` block belong to `--full`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_measures_the_headline_alone():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    # the default system and no --no-* switch: whatever --full would add, a plain run must leave out by itself
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"],
                       env=env, capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "Matom-steps/sec" and d["unit"] == "Matom-steps/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["steps"] == 5 and d["warmup"] == 2
    assert d["value"] == pytest.approx(d["config"]["atoms"] / d["ms_per_step"] / 1e3, rel=1e-3)
    assert not {"roofline", "secondary", "cpu_baseline", "host_mode_ms_per_step"} & set(d)
    assert "reneighbor_wall_ms" not in d["config"]
