"""GPU: groups through `plugin load` + `run` in the mini-host -- `fix ID GROUP nve/mdp` with `fix ID GROUP langevin/mdp`
on a strip and `minimize/mdp ... group ID`, in the fix's three modes (host-linked, `bricks yes`, `-np 4`).  The thermo
rows of a grouped NVE run are those of the mini-host's own group-aware `fix nve` to the printed digits (the convention
of tests/test_gpu_fix_nve_mdp.py); the held atoms have, in `write_dump`, the positions and velocities they were created
with, digit for digit, after every kind of run; the thermostatted run is the same in every mode."""
import os
import re

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env

pytestmark = pytest.mark.gpu
ROW_REL = 2e-7     # two 8-digit prints of one value

ALLOY = """plugin load aeamplugin.so
plugin load langevinmdpplugin.so
plugin load minimizemdpplugin.so
units metal
lattice fcc 4.045
region MeSi block 0 10 0 10 0 10
create_box 2 MeSi
create_atoms 1 region MeSi
pair_style aeam
pair_coeff * * ../tests/golden/potentials/AlSi.aeam Al Si
neighbor 1.0 bin
neigh_modify every 1 delay 0 check yes
set region MeSi type/fraction 2 0.0075 7683797
region floor block 0 10 0 10 0 2.9
region band block 0 10 4.0 7.0 0 10
group substrate region floor
group mobile subtract all substrate
group inband region band
group strip intersect inband mobile
timestep 0.001
thermo_style custom step temp etotal pe press
velocity all create 900.0 1082337
write_dump substrate custom BEFORE id x y z vx vy vz
thermo 30
"""
RUN = "run 150\nwrite_dump substrate custom AFTER id x y z vx vy vz\n"
LGV = "fix 2 strip langevin/mdp 900.0 300.0 0.05 48271\n"


def _go(script, tmp_path, tag, np_=1, env=None):
    """runs the input; (thermo rows, stdout, held atoms before, after) -- the dump rows as text"""
    before, after = tmp_path / f"{tag}.before", tmp_path / f"{tag}.after"
    rc, out, err = _run(script.replace("BEFORE", str(before)).replace("AFTER", str(after)), timeout=600, np=np_,
                        env=dict(env or {}, MDP_FIX_STATS="1"))
    assert rc == 0, err[-3000:]
    rows = lambda p: p.read_text().splitlines()[5:]   # noqa: E731
    return np.array(_thermo_rows(out)), out, rows(before), rows(after)


def _held_are_where_they_were(before, after):
    assert len(before) == 1200 == len(after)                   # six of the twenty z layers of 200 atoms
    assert before == after                                      # id x y z vx vy vz with %.17g: digit for digit
    assert all(float(v) != 0.0 for v in before[7].split()[4:])  # ... with the velocities `velocity create` drew


def _same_rows(a, b, rel=ROW_REL):
    assert a.shape == b.shape and len(a) == 6
    assert np.array_equal(a[:, 0], b[:, 0])
    for c in (1, 2, 3):                                         # temp etotal pe
        assert np.allclose(a[:, c], b[:, c], rtol=rel, atol=1e-9), (c, a[:, c], b[:, c])


@pytest.fixture(scope="module")
def host_nve(tmp_path_factory):
    """the grouped run under the mini-host's own `fix nve` in host mode: the reference of the NVE cases"""
    return _go(ALLOY + "fix 1 mobile nve\n" + RUN, tmp_path_factory.mktemp("host"), "host")


@pytest.mark.parametrize("mode", ["default", "bricks", "np4"])
def test_grouped_nve_equals_the_hosts_group_aware_fix_nve(mode, host_nve, tmp_path):
    ref, out0, b0, a0 = host_nve
    _held_are_where_they_were(b0, a0)
    assert int(re.search(r"Neighbor list builds = (\d+)", out0).group(1)) >= 1      # the run reneighbors
    fix = "fix 1 mobile nve/mdp bricks yes\n" if mode == "bricks" else "fix 1 mobile nve/mdp\n"
    rows, out, before, after = _go(ALLOY + fix + RUN, tmp_path, mode, np_=4 if mode == "np4" else 1,
                                   env=_double_env() if mode == "np4" else None)
    if mode == "default":
        assert int(re.search(r"Neighbor list builds = (\d+)", out).group(1)) >= 1  # host reneighborings re-upload the mask
    else:
        m = re.search(r"fix nve/mdp: (\d+) bricks, (\d+) reneighborings on the device", out)
        assert int(m.group(1)) == (4 if mode == "np4" else 1) and int(m.group(2)) >= 1
    _same_rows(rows, ref)
    assert before == b0
    _held_are_where_they_were(before, after)
    assert rows[-1, 1] < 0.8 * rows[0, 1]                       # (the lattice takes up half the kinetic energy: atoms moved)


def test_langevin_on_a_strip_is_the_same_run_in_every_mode(tmp_path):
    """`fix 1 mobile nve/mdp` + `fix 2 strip langevin/mdp`: the noise is keyed by tag and step and the strip by the mask
    that travels with the atoms, so host-linked, `bricks yes` and four ranks print the same rows; the substrate stays"""
    runs = {}
    for mode in ("default", "bricks", "np4"):
        fix = "fix 1 mobile nve/mdp bricks yes\n" if mode == "bricks" else "fix 1 mobile nve/mdp\n"
        runs[mode] = _go(ALLOY + fix + LGV + RUN, tmp_path, mode, np_=4 if mode == "np4" else 1,
                         env=_double_env() if mode == "np4" else None)
        _held_are_where_they_were(runs[mode][2], runs[mode][3])
    _same_rows(runs["bricks"][0], runs["default"][0])
    _same_rows(runs["np4"][0], runs["bricks"][0])
    nve, _, _, _ = _go(ALLOY + "fix 1 mobile nve/mdp\n" + RUN, tmp_path, "nve")
    assert abs(runs["default"][0][-1, 2] - nve[-1, 2]) > 1.0   # the thermostat exchanged energy: etotal left the NVE run's


def test_minimize_mdp_on_a_group_holds_the_rest(tmp_path):
    """`minimize/mdp ... group mobile`: the substrate stays where it was, with its velocities; the energy goes down"""
    before, after = tmp_path / "min.before", tmp_path / "min.after"
    script = (ALLOY + "minimize/mdp 0.0 1.0e-4 300 3000 group mobile\nwrite_dump substrate custom AFTER id x y z vx vy vz\n"
              "write_dump mobile custom MOBILE id x y z vx vy vz\n")
    rc, out, err = _run(script.replace("BEFORE", str(before)).replace("AFTER", str(after)).replace("MOBILE", str(tmp_path / "mobile")),
                        timeout=600)
    assert rc == 0, err[-3000:]
    e = [float(v) for v in re.search(r"Energy initial, next-to-last, final = \n\s+(\S+)\s+(\S+)\s+(\S+)", out).groups()]
    assert e[2] < e[0] - 0.1, e                                 # (the Si atoms sit on unrelaxed Al sites)
    fn = [float(v) for v in re.search(r"Force two-norm initial, final = (\S+) (\S+)", out).groups()]
    assert fn[1] < fn[0]
    _held_are_where_they_were(before.read_text().splitlines()[5:], after.read_text().splitlines()[5:])
    mobile = [l.split() for l in (tmp_path / "mobile").read_text().splitlines()[5:]]
    assert len(mobile) == 2800
    assert max(abs(float(v)) for r in mobile for v in r[4:]) < 5.0   # the moving atoms lost the 900 K they were given


def test_rebomos_host_linked_group_run_equals_the_hosts_fix_nve(tmp_path):
    """the clamped MoS2 example: host-linked, the device reads atom->mask through its own permutation of the host's order"""
    text = open(os.path.join(PKG, "examples", "in.rebomos-clamped.group-mdp.mi355x")).read()
    heat = "fix heat strip langevin/mdp 300.0 300.0 0.1 48271 zero yes tally yes\n"
    assert heat in text and "f_heat econserve" in text and "run 500" in text
    text = text.replace(heat, "").replace(" f_heat econserve", "").replace("run 500", "run 200")
    text = text.replace("velocity all create 300.0", "velocity all create 1500.0").replace("neighbor 1.0 bin", "neighbor 0.4 bin")
    text = text.replace("write_dump clamped custom clamped.dump", f"write_dump clamped custom {tmp_path / 'after'}")
    text = text.replace("thermo 50\n", f"thermo 50\nwrite_dump clamped custom {tmp_path / 'before'} id x y z vx vy vz\n")
    rc0, out0, err0 = _run(text.replace("fix integrate mobile nve/mdp", "fix integrate mobile nve"), timeout=600)
    assert rc0 == 0, err0[-3000:]
    held0 = (tmp_path / "after").read_text().splitlines()[5:]
    rc1, out1, err1 = _run(text, timeout=600)
    assert rc1 == 0, err1[-3000:]
    held1 = (tmp_path / "after").read_text().splitlines()[5:]
    start = (tmp_path / "before").read_text().splitlines()[5:]
    assert len(start) == 576 and start == held0 == held1       # a quarter of the 2 304 atoms, all velocities set to 0
    assert int(re.search(r"Neighbor list builds = (\d+)", out1).group(1)) >= 2
    r0, r1 = _thermo_rows(out0), _thermo_rows(out1)
    assert [int(r[0]) for r in r1] == [0, 50, 100, 150, 200]
    for a, b in zip(r0, r1):                                    # step temp pe ke
        assert a[1] == pytest.approx(b[1], rel=2e-7)
        assert a[2] == pytest.approx(b[2], rel=2e-8)
        assert a[3] == pytest.approx(b[3], rel=2e-7)
