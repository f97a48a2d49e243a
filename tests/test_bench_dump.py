"""bench.py --dump-outputs: the arrays of the last timed step, in tag order whatever order the device keeps its atoms
in, the same seeded sample from run to run, float64, within 64 MB; several ranks' atoms put together on rank 0.
The domain here is a stand-in with the calls dump_outputs makes of resident.DeviceDomain (the GPU runs of the real
path are bench.py's own)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _System:
    def __init__(self, n):
        self.n = n
        self.tag = np.arange(1, n + 1, dtype=np.int32)


class _Ctx:
    def __init__(self, tags, x, v, f):
        self.tags, self.arrs = tags, dict(x=x, v=v, f=f)

    def md_download(self, nlocal, want=("x", "v", "f")):
        assert nlocal == len(self.tags)
        return {k: (self.arrs[k].copy() if k in want else None) for k in ("x", "v", "f")} | {"eatom": None}


class _Domain:
    """owned atoms of one rank in a shuffled storage order; x/v/f are functions of the tag"""
    def __init__(self, tags):
        t = tags.astype(np.float64)[:, None]
        self.nlocal = len(tags)
        self.tags_local = tags.astype(np.int32)
        self.ctx = _Ctx(tags, t * [1.0, 2.0, 3.0], t * [-1.0, 0.5, 0.25], t * [7.0, -3.0, 1e-3])

    def thermo(self):
        return dict(pe=-12.5, ke=3.0, virial=np.arange(6.0))


class _Dist:
    """all_gather_object over ranks whose parts were computed beforehand"""
    def __init__(self, parts):
        self.parts = parts

    def all_gather_object(self, out, obj):
        out[:] = self.parts


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}


def test_dump_is_tag_ordered_seeded_and_bounded(tmp_path):
    n = 3 * bench.DUMP_SAMPLE_ATOMS
    s = _System(n)
    rng = np.random.default_rng(1)
    par = dict(dist=None, world=1, rank=0)
    infos = []
    for run in range(2):                            # another storage order each run: the same file contents
        d = str(tmp_path / f"run{run}")
        infos.append(bench.dump_outputs(_Domain(rng.permutation(s.tag)), s, d, 110, True, par))
        got = _load(d)
        assert set(got) == {"tags", "positions", "velocities", "forces", "energy_virial"}
        assert all(a.dtype == np.float64 for a in got.values())
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        t = got["tags"]
        assert len(t) == bench.DUMP_SAMPLE_ATOMS and np.all(np.diff(t) > 0)
        np.testing.assert_array_equal(got["positions"], t[:, None] * [1.0, 2.0, 3.0])
        np.testing.assert_array_equal(got["forces"], t[:, None] * [7.0, -3.0, 1e-3])
        np.testing.assert_array_equal(got["energy_virial"], [-12.5, 0, 1, 2, 3, 4, 5])
    a, b = _load(str(tmp_path / "run0")), _load(str(tmp_path / "run1"))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert infos[0]["atoms_dumped"] == bench.DUMP_SAMPLE_ATOMS and infos[0]["step"] == 110


def test_small_system_is_dumped_whole_and_energy_only_on_thermo_steps(tmp_path):
    s = _System(1000)
    d = str(tmp_path / "d")
    info = bench.dump_outputs(_Domain(s.tag[::-1].copy()), s, d, 7, False, dict(dist=None, world=1, rank=0))
    got = _load(d)
    assert "energy_virial" not in got and info["sample_seed"] is None
    np.testing.assert_array_equal(got["tags"], np.arange(1, 1001))
    np.testing.assert_array_equal(got["velocities"], got["tags"][:, None] * [-1.0, 0.5, 0.25])


def test_ranks_are_put_together_on_rank_zero(tmp_path):
    s = _System(5000)
    perm = np.random.default_rng(2).permutation(s.tag)
    doms = [_Domain(perm[:1700]), _Domain(perm[1700:])]
    parts = []
    for dm in doms:                                  # what each rank contributes
        t = dm.tags_local.astype(np.int64)
        parts.append((t, dm.ctx.arrs["x"], dm.ctx.arrs["v"], dm.ctx.arrs["f"]))
    dist = _Dist(parts)
    assert bench.dump_outputs(doms[1], s, str(tmp_path / "r1"), 5, True, dict(dist=dist, world=2, rank=1)) is None
    assert not (tmp_path / "r1").exists()
    bench.dump_outputs(doms[0], s, str(tmp_path / "r0"), 5, True, dict(dist=dist, world=2, rank=0))
    got = _load(str(tmp_path / "r0"))
    np.testing.assert_array_equal(got["tags"], np.arange(1, 5001))
    np.testing.assert_array_equal(got["positions"], got["tags"][:, None] * [1.0, 2.0, 3.0])


def test_steps_below_one_are_refused():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr and '"metric"' not in r.stdout
