"""GPU: several `fix langevin/mdp` baths through `plugin load` + `run` in the mini-host, handing their thermostats to one
`fix nve/mdp` (its Fix::extract("mdp_langevin_baths") block): a hot and a cold strip of the alloy cell of the group tests
above a held floor.  The two fixes in either input order, the default (host-linked) mode against `bricks yes`, `ecouple`
against f_hot + f_cold, one bath on a strip against two baths on its halves, 2 ranks against one, the shipped example, and
the refusals (shared atoms, fix nvt/mdp next to two baths)."""
import numpy as np
import pytest

from test_plugin_boundary import _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env

pytestmark = pytest.mark.gpu
ROW_REL = 2e-7     # two 8-digit prints of one value

ALLOY = """plugin load aeamplugin.so
plugin load langevinmdpplugin.so
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
region lowband block 0 10 1.0 4.0 0 10
region highband block 0 10 6.0 9.0 0 10
region lefthalf block 0 4.9 0 10 0 10
group substrate region floor
group mobile subtract all substrate
group inlow region lowband
group inhigh region highband
group inleft region lefthalf
group hotstrip intersect inlow mobile
group coldstrip intersect inhigh mobile
group hotleft intersect hotstrip inleft
group hotright subtract hotstrip hotleft
timestep 0.001
thermo_style custom step temp pe ke f_hot f_cold ecouple econserve
velocity all create 300.0 1082337
thermo 30
"""
NVE = "fix integrate mobile nve/mdp\n"
HOT = "fix hot hotstrip langevin/mdp 900.0 900.0 0.05 48271 tally yes\n"
COLD = "fix cold coldstrip langevin/mdp 100.0 100.0 0.05 7919 tally yes zero yes\n"
RUN = "run 150\n"


def _rows(script, np_=1, env=None):
    rc, out, err = _run(script, timeout=600, np=np_, env=env)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert len(rows) == 6 and rows[-1, 0] == 150
    return rows, out


@pytest.fixture(scope="module")
def default_rows():
    return _rows(ALLOY + NVE + HOT + COLD + RUN)[0]


def test_the_two_baths_exchange_heat_and_ecouple_is_their_sum(default_rows):
    r = default_rows
    f_hot, f_cold, ecouple, econserve = r[:, 4], r[:, 5], r[:, 6], r[:, 7]
    assert f_hot[-1] < -1.0 and f_cold[-1] > 0.1, (f_hot, f_cold)      # heat goes in at the hot strip and out at the cold one
    for a, b, c in zip(f_hot, f_cold, ecouple):                         # ... to the printed digits
        assert abs(c - (a + b)) <= ROW_REL * (abs(a) + abs(b) + abs(c)), (a, b, c)
    assert np.allclose(econserve, r[:, 2] + r[:, 3] + ecouple, rtol=ROW_REL)
    assert np.ptp(econserve) < 0.02 * abs(f_hot[-1])                    # the tallies account for what the baths exchanged


def test_the_input_order_of_the_fixes_does_not_matter(default_rows):
    """cold before hot, and both before the integrator: the bath slots follow Modify's list, the thermo rows do not change"""
    b, _ = _rows(ALLOY + COLD + HOT + NVE + RUN)
    assert np.array_equal(default_rows, b)
    c, _ = _rows(ALLOY + COLD + NVE + HOT + RUN)
    assert np.array_equal(default_rows, c)


def test_default_mode_agrees_with_bricks_yes(default_rows):
    b, _ = _rows(ALLOY + NVE.replace("nve/mdp", "nve/mdp bricks yes") + HOT + COLD + RUN)
    assert default_rows.shape == b.shape
    for c in (1, 2, 3):                                                 # temp pe ke
        assert np.allclose(default_rows[:, c], b[:, c], rtol=ROW_REL, atol=1e-9), (c, default_rows[:, c], b[:, c])
    for c in (4, 5, 6):                                                 # the tallies: sums in another atom order
        assert np.allclose(default_rows[:, c], b[:, c], rtol=ROW_REL, atol=1e-6), (c, default_rows[:, c], b[:, c])


def test_one_bath_on_a_strip_equals_two_baths_on_its_halves():
    """the same numbers and seed, `zero no`: the noise of an atom hangs on its tag, so the pe and ke columns are identical"""
    one = "fix hot hotstrip langevin/mdp 900.0 300.0 0.05 48271 tally yes\n"
    two = ("fix hot hotleft langevin/mdp 900.0 300.0 0.05 48271 tally yes\n"
           "fix cold hotright langevin/mdp 900.0 300.0 0.05 48271 tally yes\n")
    style = "thermo_style custom step temp pe ke f_hot ecouple\n"
    a, _ = _rows(ALLOY + style + NVE.replace("nve/mdp", "nve/mdp bricks yes") + one + RUN)
    b, _ = _rows(ALLOY + style + NVE.replace("nve/mdp", "nve/mdp bricks yes") + two + RUN)
    assert np.array_equal(a[:, 1:4], b[:, 1:4])
    assert abs(a[-1, 4]) > 1.0 and abs(b[-1, 4]) > 0.2 and abs(b[-1, 4]) < abs(a[-1, 4])
    assert np.allclose(a[:, 5], b[:, 5], rtol=ROW_REL, atol=1e-6)       # ecouple: the two halves add up to the one


def test_two_ranks_without_a_tally_follow_the_one_rank_run():
    style = "thermo_style custom step temp pe ke\n"
    hot, cold = HOT.replace(" tally yes", ""), COLD.replace(" tally yes zero yes", "")
    one, _ = _rows(ALLOY + style + NVE.replace("nve/mdp", "nve/mdp bricks yes") + hot + cold + RUN)
    two, out = _rows(ALLOY + style + NVE + hot + cold + RUN, np_=2, env=_double_env())
    assert "fix nve/mdp: 2 bricks" in out
    assert one.shape == two.shape
    for a, b in zip(two, one):
        assert a[0] == b[0]
        for u, v in zip(a[1:], b[1:]):
            assert u == pytest.approx(v, rel=2e-8, abs=1e-6)


def test_the_example_runs_and_its_baths_work_against_each_other():
    rc, out, err = _run(script_file="examples/in.rebomos-ribbon.nemd-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    r = np.array(_thermo_rows(out))
    assert r[-1, 0] == 1000
    f_hot, f_cold, ecouple, econserve = r[:, 4], r[:, 5], r[:, 6], r[:, 7]
    assert f_hot[-1] < 0.0 < f_cold[-1], (f_hot[-1], f_cold[-1])
    assert np.ptp(econserve) < 0.05 * (abs(f_hot[-1]) + abs(f_cold[-1]))
    # seven eighths of bin 3 are hot-strip atoms (held at 400 K for twenty coupling times), seven eighths of bin 10
    # cold-strip atoms (200 K): about 175 K apart, and a bin of ~290 atoms reads its temperature to 5 % (sqrt(2 / 3N))
    assert np.mean(r[-3:, 8]) > np.mean(r[-3:, 12]) + 100.0, (r[-3:, 8], r[-3:, 12])


def test_shared_atoms_are_refused_with_both_fixes_named():
    rc, out, err = _run(ALLOY + NVE + HOT + "fix cold hotleft langevin/mdp 100.0 100.0 0.05 7919\n" + RUN, timeout=300)
    assert rc == 1
    assert "fixes hot and cold share" in err and "(groups hotstrip and hotleft)" in err and "must be disjoint" in err, err[-2000:]
    rc, out, err = _run(ALLOY + NVE + HOT + "fix cold mobile langevin/mdp 100.0 100.0 0.05 7919\n" + RUN, timeout=300)
    assert rc == 1 and "fixes hot and cold share" in err, err[-2000:]   # the integrator's own group next to another bath


def test_atoms_added_to_a_group_after_the_fixes_are_refused_at_run():
    """the groups were disjoint when the fixes were defined; `group` then adds the hot strip's atoms to the cold one's group:
    init() looks again"""
    rc, out, err = _run(ALLOY + NVE + HOT + COLD + "group coldstrip intersect inlow mobile\n" + RUN, timeout=300)
    assert rc == 1
    assert "fixes hot and cold share" in err and "(groups hotstrip and coldstrip)" in err and "must be disjoint" in err, err[-2000:]


def test_nvt_mdp_next_to_two_baths_is_still_a_second_thermostat():
    text = (ALLOY.replace("plugin load langevinmdpplugin.so\n", "plugin load langevinmdpplugin.so\nplugin load nvtmdpplugin.so\n")
            + "fix integrate all nvt/mdp temp 300.0 300.0 0.1\n" + HOT + COLD + RUN)
    rc, out, err = _run(text, timeout=300)
    assert rc == 1 and "use one thermostat" in err, err[-2000:]
