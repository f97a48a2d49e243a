"""GPU: `compute cna/atom/mdp` through `plugin load` + `run` in the mini-host, read through `dump custom`, the thermo's c_ID[k]
and `compute reduce`: the close-packed stack of tests/cnaref.py (ABCABCABABAB as a custom lattice of 24 basis atoms, 960 atoms,
half fcc and half hcp) at 50 K on 1, 2 and 8 ranks; the dumped column against the library's own read of the dumped positions
and against the NumPy reference; the census at step 0; the warning about more than 16 neighbours; the refusals that need a
run to be seen; and the example."""
import glob
import os

import numpy as np
import pytest

from lammps_plugins_amd.host import capi, resident, system as S
from test_plugin_boundary import PKG, _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env
from test_gpu_rdf_mdp import _by_tag, _context
from test_gpu_struct_mdp_plugin import _read_dump
import cnaref

pytestmark = pytest.mark.gpu

PER = (1, 1, 1)
RC = "3.4528"                                 # 0.8536 a
NX, NY = 8, 5

DECK = """plugin load aeamplugin.so
plugin load cnamdpplugin.so
units metal
LATTICE
region cell block 0 %d 0 %d 0 1
create_box 2 cell
create_atoms 1 box
pair_style aeam
pair_coeff * * ../tests/golden/potentials/AlSi.aeam Al Si
neighbor 1.0 bin
neigh_modify every 1 delay 0 check yes
timestep 0.001
velocity all create 50.0 1082337
FIX
COMPUTES
thermo 10
run 10
""" % (NX, NY)
BRICKS = "fix 1 all nve/mdp bricks yes"
COLS = "id type x y z c_cna"


def _deck(computes, fix=BRICKS):
    return DECK.replace("LATTICE", cnaref.stack_lattice()).replace("FIX", fix).replace("COMPUTES", computes)


def _stack_computes(tmp):
    return (f"compute cna all cna/atom/mdp {RC}\ncompute top all reduce max c_cna\ncompute low all reduce min c_cna\n"
            f"dump d all custom 10 {tmp}/s.*.dump {COLS}\nthermo_style custom step c_cna[1] c_cna[2] c_cna[3] c_cna[4] c_cna[5] c_top c_low\n")


@pytest.fixture(scope="module")
def stack_runs(tmp_path_factory):
    out = {}
    for np_ in (1, 2, 8):
        tmp = tmp_path_factory.mktemp(f"np{np_}")
        rc, so, err = _run(_deck(_stack_computes(tmp)), timeout=300, np=np_, env=_double_env() if np_ > 1 else None)
        assert rc == 0, err[-3000:]
        assert "Too many neighbors" not in err
        out[np_] = dict(thermo=np.array(_thermo_rows(so)), dump=_read_dump(f"{tmp}/s.10.dump"))
    return out


def test_the_census_in_the_thermo(stack_runs):
    """c_ID[1] and c_ID[2] are 480 and 480 at step 0 (and after ten steps at 50 K), nothing is bcc, icosahedral or other, and
    compute reduce max / min over the per-atom vector give 2 and 1 -- on 1, 2 and 8 ranks alike"""
    for np_, run in stack_runs.items():
        rows = run["thermo"]
        assert rows[:, 0].tolist() == [0, 10], np_
        for row in rows:
            assert row[1:].tolist() == [480, 480, 0, 0, 0, 2, 1], (np_, row)


def test_the_dump_column_is_the_librarys_and_the_references(stack_runs, capsys):
    """the dump of step 10 on one rank, sorted by id with x, y, z printed with %.17g: the column equals what the library reads from
    a context that holds those positions, by ID, and what the NumPy reference makes of them"""
    step, cols, rows = stack_runs[1]["dump"]
    assert step == 10 and cols == COLS.split() and len(rows) == 960 and rows[:, 0].tolist() == list(range(1, 961))
    x, col = rows[:, 2:5], rows[:, 5].astype(np.int64)
    h = cnaref.stack_cell(0.0)[1]
    ref = cnaref.cna(x, h, PER, float(RC))
    assert not ref["ambiguous"].any() and np.array_equal(col, ref["pattern"])
    assert cnaref.histogram(col).tolist() == [0, 480, 480, 0, 0, 0]
    box = S.Box(np.zeros(3), h.diagonal().copy(), np.zeros(3))
    mass = np.array([0.0] + list(capi.AeamFile(os.path.join(PKG, "../tests/golden/potentials/AlSi.aeam")).mass[:2]))
    s = S.System(box, S.wrap(box, x), rows[:, 1].astype(np.int32), np.arange(1, 961, dtype=np.int32), mass)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        d.cna(float(RC))
        d.compute(0, 0)
        tags, val = d.cna_read()
        assert np.array_equal(_by_tag(960, tags, val).astype(np.int64), col)
        assert ctx.cna_counts().tolist() == [0, 480, 480, 0, 0, 0]
    finally:
        ctx.close()
    layer = np.rint((x[:, 2] - x[:, 2].min()) / (h[2, 2] / 12)).astype(int) % 12
    with capsys.disabled():
        print(f"stack, step 10: fcc layers {sorted(set(layer[col == 1].tolist()))}, hcp layers {sorted(set(layer[col == 2].tolist()))}")
    assert len(set(layer[col == 1].tolist())) == 6 and not set(layer[col == 1].tolist()) & set(layer[col == 2].tolist())


def test_one_two_and_eight_ranks_dump_the_same_rows(stack_runs):
    a = stack_runs[1]["dump"][2]
    for np_ in (2, 8):
        step, cols, b = stack_runs[np_]["dump"]
        assert step == 10 and cols == COLS.split()
        assert np.array_equal(a[:, :2], b[:, :2]) and np.array_equal(a[:, 5], b[:, 5]) and np.abs(a[:, 2:5] - b[:, 2:5]).max() < 1e-9
        assert np.array_equal(stack_runs[1]["thermo"], stack_runs[np_]["thermo"])


def test_more_than_16_neighbours_warn_and_go_on(tmp_path):
    """Rc = 4.2 takes the six second neighbours in: every atom is `other`, the run goes on, and each evaluation prints LAMMPS'
    warning with the number of atoms"""
    computes = "compute cna all cna/atom/mdp 4.2\nthermo_style custom step c_cna[1] c_cna[2] c_cna[5]\n"
    rc, so, err = _run(_deck(computes), timeout=300)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(so))
    assert rows[:, 0].tolist() == [0, 10] and np.all(rows[:, 1:3] == 0) and np.all(rows[:, 3] == 960)
    assert err.count("WARNING: Too many neighbors in CNA for 960 atoms") == 2, err[-2000:]


@pytest.mark.parametrize("fix,compute,msg", [
    ("fix 1 all nve", "compute a all cna/atom/mdp 3.45", "Compute cna/atom/mdp requires fix nve/mdp"),
    ("fix 1 all nve/mdp", "compute a all cna/atom/mdp 3.45",
     "runs in the host-linked mode, where the host's atom->x and neighbour list are current: use compute cna/atom"),
    (BRICKS, "compute a all cna/atom/mdp 25", "Compute cna/atom/mdp: the cutoff 25 is beyond the pair style's cutforce"),
    (BRICKS, "compute a all cna/atom/mdp 6.51", "the cutoff 6.51 is beyond the pair style's cutforce"),
])
def test_refusals_that_need_a_run(fix, compute, msg):
    rc, out, err = _run(_deck(compute + "\nthermo_style custom step c_a[1]\n", fix), timeout=300)
    assert rc == 1
    assert msg in err, err[-2000:]


def test_the_example_runs(capsys):
    """examples/in.aeam-alsi.cna-mdp.mi355x: the alloy with a vacancy; every thermo row counts fcc + hcp + other = the atoms, the
    vacancy's twelve neighbours are among the `other`, and the dump's column adds up to the thermo's census"""
    for f in glob.glob(os.path.join(PKG, "alsi.cna.*.dump")):
        os.remove(f)
    rc, out, err = _run(script_file="examples/in.aeam-alsi.cna-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 50, 100, 150, 200] and rows.shape[1] == 6
    with capsys.disabled():
        print(f"alsi.cna: fcc {rows[:, 3].tolist()}, hcp {rows[:, 4].tolist()}, other {rows[:, 5].tolist()}")
    assert rows[0, 3:].tolist() == [2035, 0, 12] and np.all(rows[:, 5] >= 12) and np.all(rows[:, 3] + rows[:, 4] + rows[:, 5] <= 2047)
    _, cols, d = _read_dump(os.path.join(PKG, "alsi.cna.200.dump"))
    assert cols == "id type x y z c_cna".split() and len(d) == 2047
    hist = cnaref.histogram(d[:, 5])
    assert hist[0] == 0 and [hist[1], hist[2], hist[5]] == rows[-1, 3:].tolist()
