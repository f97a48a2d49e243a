"""GPU: `compute coord/atom/mdp` and `compute centro/atom/mdp` through `plugin load` + `run` in the mini-host, read through
`dump custom` and `compute reduce`: the hot alloy with one atom removed on 1 and 2 ranks, every dumped file against
tests/structref.py on that file's own x, y, z (printed with %.17g: the positions the device read); the MoS2 cell, where every
Mo keeps its 6 S; dump steps that are no thermo steps; the refusals that need a run to be seen; and the two examples."""
import glob
import os

import numpy as np
import pytest

from test_plugin_boundary import PKG, _run, _thermo_rows
from test_gpu_minilmp_ranks import _double_env
import structref

pytestmark = pytest.mark.gpu

PER = (1, 1, 1)
A = 4.045
H_ALLOY = np.diag([6 * A] * 3)
RC = 6.5                                      # the alloy's cutforce: the default cutoff of centro/atom/mdp
PRINTED = 6e-8                                # a thermo column is %.8g: half a unit of the eighth digit is at most 5e-8 of the value

HOT = """plugin load aeamplugin.so
plugin load coordmdpplugin.so
plugin load centromdpplugin.so
units metal
lattice fcc 4.045
region MeSi block 0 6 0 6 0 6
create_box 2 MeSi
create_atoms 1 region MeSi
pair_style aeam
pair_coeff * * ../tests/golden/potentials/AlSi.aeam Al Si
neighbor 1.0 bin
neigh_modify every 1 delay 0 check yes
set region MeSi type/fraction 2 0.05 7683797
group gone id 432
delete_atoms group gone
timestep 0.001
velocity all create 2500.0 1082337
group al type 1
FIX
compute cs all centro/atom/mdp fcc
compute nn all coord/atom/mdp cutoff 3.5 * 1 2
compute na al coord/atom/mdp cutoff 3.5
compute csmax all reduce max c_cs
compute nnsum all reduce sum c_nn[1]
compute namin al reduce min c_na
compute naave al reduce ave c_na
DUMP
thermo_style custom step c_csmax c_nnsum c_namin c_naave
thermo THERMO
run 30
"""
BRICKS = "fix 1 all nve/mdp bricks yes"
COLS = "id type x y z c_cs c_nn[1] c_nn[2] c_nn[3] c_na"


def _deck(tmp, every=10, thermo=10, fix=BRICKS):
    return (HOT.replace("FIX", fix).replace("DUMP", f"dump d all custom {every} {tmp}/s.*.dump {COLS}").replace("THERMO", str(thermo)))


def _read_dump(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "ITEM: TIMESTEP" and lines[2] == "ITEM: NUMBER OF ATOMS" and lines[4].startswith("ITEM: ATOMS ")
    cols = lines[4].split()[2:]
    rows = np.array([[float(t) for t in l.split()] for l in lines[5:]])
    assert len(rows) == int(lines[3]) and rows.shape[1] == len(cols)
    return int(lines[1]), cols, rows


def _check_file(path, capsys):
    """one snapshot of the hot alloy against structref on its own positions; returns (step, rows)"""
    step, cols, rows = _read_dump(path)
    assert cols == COLS.split() and len(rows) == 863 and rows[:, 0].tolist() == list(range(1, 864))      # sorted by id
    types, x = rows[:, 1].astype(int), rows[:, 2:5]
    al = types == 1
    zref = structref.centro(x, H_ALLOY, PER, 12, RC)
    assert int(zref["ambiguous"].sum()) <= 2
    ok = ~zref["ambiguous"]
    bound = structref.centro_bound(12, RC, 6 * A)
    err = np.abs(rows[:, 5] - zref["value"])[ok]
    cref = structref.coord(x, types, H_ALLOY, PER, 3.5, [(1, 2), (1, 1), (2, 2)])
    aref = structref.coord(x, types, H_ALLOY, PER, 3.5, [(1, 2)], al)
    assert cref["n_edge"] <= 2 and aref["n_edge"] <= 2
    with capsys.disabled():
        print(f"{os.path.basename(path)}: centro worst |dump - reference| {err.max():.2e} A^2 (bound {bound:.2e}), max {rows[:, 5].max():.3f} A^2; "
              f"coord {cref['n_edge']} edge pairs, {int(rows[:, 6].sum())} partners")
    assert err.max() <= bound
    for dev, ref in ((rows[:, 6:9], cref), (rows[:, 9:10], aref)):
        assert np.all((dev >= ref["count_sure"]) & (dev <= ref["count_sure"] + ref["edge"]))
    assert np.all(rows[~al, 9] == 0.0) and rows[al, 9].min() >= 5 and (~al).sum() > 20        # outside group al: exactly 0
    return step, rows


@pytest.fixture(scope="module")
def hot_runs(tmp_path_factory):
    out = {}
    for np_ in (1, 2):
        tmp = tmp_path_factory.mktemp(f"np{np_}")
        rc, so, err = _run(_deck(tmp), timeout=600, np=np_, env=_double_env() if np_ > 1 else dict(MDP_FIX_STATS="1"))
        assert rc == 0, err[-3000:]
        assert "Deleted 1 atoms, new total = 863" in so
        out[np_] = dict(tmp=tmp, thermo=np.array(_thermo_rows(so)))
    return out


@pytest.mark.parametrize("np_", [1, 2])
def test_every_dumped_file_matches_the_reference_on_its_own_positions(hot_runs, np_, capsys):
    """`dump ... 10` over 30 steps writes steps 10, 20 and 30 (no snapshot of the setup: the atoms are in the host's own order
    there); `-np 2` writes one file per step with the rows of both ranks.  `compute reduce` in the thermo row of the same step
    equals the dump's figures to the 8 printed digits."""
    run = hot_runs[np_]
    files = sorted(glob.glob(f"{run['tmp']}/s.*.dump"), key=lambda p: int(p.split(".")[-2]))
    assert [int(p.split(".")[-2]) for p in files] == [10, 20, 30]
    thermo = {int(r[0]): r for r in run["thermo"]}
    assert sorted(thermo) == [0, 10, 20, 30]
    for path in files:
        step, rows = _check_file(path, capsys)
        al = rows[:, 1] == 1
        t = thermo[step]
        assert t[1] == pytest.approx(rows[:, 5].max(), rel=PRINTED) and t[1] > 1.0
        assert t[2] == rows[:, 6].sum() and t[3] == rows[al, 9].min() and t[4] == pytest.approx(rows[al, 9].mean(), rel=PRINTED)


def test_one_and_two_ranks_dump_the_same_rows(hot_runs, capsys):
    """the same input on -np 1 and -np 2, by id: coord is equal and centro within the bound, at every dumped step"""
    bound = structref.centro_bound(12, RC, 6 * A)
    for step in (10, 20, 30):
        a = _read_dump(f"{hot_runs[1]['tmp']}/s.{step}.dump")[2]
        b = _read_dump(f"{hot_runs[2]['tmp']}/s.{step}.dump")[2]
        with capsys.disabled():
            print(f"step {step}: |dx| {np.abs(a[:, 2:5] - b[:, 2:5]).max():.2e} A, |d centro| {np.abs(a[:, 5] - b[:, 5]).max():.2e} A^2, "
                  f"{int((a[:, 6:] != b[:, 6:]).sum())} counts differ")
        assert np.array_equal(a[:, :2], b[:, :2]) and np.array_equal(a[:, 6:], b[:, 6:])
        assert np.abs(a[:, 5] - b[:, 5]).max() <= bound


def test_dump_steps_that_are_not_thermo_steps(tmp_path, capsys):
    """`dump 7` with `thermo 10`: steps 7, 14, 21 and 28 are output steps for the dump alone (Output::next is the smaller of the two),
    the atoms come home for them, and every file is right; the thermo rows are those of thermo 10"""
    rc, so, err = _run(_deck(tmp_path, every=7), timeout=600, env=dict(MDP_FIX_STATS="1"))
    assert rc == 0, err[-3000:]
    files = sorted(glob.glob(f"{tmp_path}/s.*.dump"), key=lambda p: int(p.split(".")[-2]))
    assert [int(p.split(".")[-2]) for p in files] == [7, 14, 21, 28]
    for path in files:
        _check_file(path, capsys)
    assert [int(r[0]) for r in _thermo_rows(so)] == [0, 10, 20, 30]


MOS2 = """plugin load rebomosplugin.so
plugin load coordmdpplugin.so
plugin load centromdpplugin.so
units metal
lattice custom 1.0 &
    a1  3.1903157234 0.0000000000  0.0000000000 &
    a2 -1.5964590311 2.7651481541  0.0000000000 &
    a3  0.0000000000 0.0000000000 13.9827680588 &
    basis 0.0 0.0 $(3.0/4.0) &
    basis 0.0 0.0 $(1.0/4.0) &
    basis $(2.0/3.0) $(1.0/3.0) 0.862008989 &
    basis $(1.0/3.0) $(2.0/3.0) 0.137990996 &
    basis $(1.0/3.0) $(2.0/3.0) 0.362008989 &
    basis $(2.0/3.0) $(1.0/3.0) 0.637991011 &
    origin 0.1 0.1 0.1
region cell prism 0 4 0 8 0 1 -2.0 0.0 0.0
create_box 2 cell
create_atoms 2 box basis 1 1 basis 2 1 basis 3 2 basis 4 2 basis 5 2 basis 6 2
mass 1 95.95
mass 2 32.065
pair_style rebomos
pair_coeff * * ../tests/golden/potentials/MoS.REBO.set5b M S
velocity all create 300.0 4928459
group Mo type 1
group S type 2
FIX
COMPUTES
thermo 25
run 50
"""


def test_every_mo_keeps_its_six_sulphurs(tmp_path):
    """`coord/atom/mdp cutoff 2.8 2` on group Mo at 300 K: 6 for every Mo, in the dump (which holds the Mo rows alone) and in the
    thermo; an S has 3 Mo; centro/atom/mdp at its default cutoff is refused on MoS2 with a message that names cutoff"""
    computes = (f"compute nS Mo coord/atom/mdp cutoff 2.8 2\ncompute nMo S coord/atom/mdp cutoff 2.8 1\n"
                f"compute lo Mo reduce min c_nS\ncompute hi Mo reduce max c_nS\ncompute s3 S reduce ave c_nMo\n"
                f"dump d Mo custom 25 {tmp_path}/mo.*.dump id type c_nS\nthermo_style custom step c_lo c_hi c_s3\n")
    rc, so, err = _run(MOS2.replace("FIX", "fix 1 all nve/mdp bricks yes").replace("COMPUTES", computes), timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(so))
    assert rows[:, 0].tolist() == [0, 25, 50] and np.all(rows[:, 1:3] == 6.0) and np.all(rows[:, 3] == 3.0)
    for step in (25, 50):
        _, cols, d = _read_dump(f"{tmp_path}/mo.{step}.dump")
        assert cols == ["id", "type", "c_nS"] and len(d) == 96 and np.all(d[:, 1] == 1) and np.all(d[:, 2] == 6.0)
    computes = "compute cs all centro/atom/mdp 6\ncompute m all reduce max c_cs\nthermo_style custom step c_m\n"
    rc, so, err = _run(MOS2.replace("FIX", "fix 1 all nve/mdp bricks yes").replace("COMPUTES", computes), timeout=600)
    assert rc == 1
    assert "more than 128 atoms inside the cutoff" in err and "use a smaller cutoff" in err, err[-2000:]


@pytest.mark.parametrize("fix,compute,msg", [
    ("fix 1 all nve", "compute a all coord/atom/mdp cutoff 2.8", "Compute coord/atom/mdp requires fix nve/mdp"),
    ("fix 1 all nve", "compute a all centro/atom/mdp 6 cutoff 4.0", "Compute centro/atom/mdp requires fix nve/mdp"),
    ("fix 1 all nve/mdp", "compute a all coord/atom/mdp cutoff 2.8",
     "runs in the host-linked mode, where the host's atom->x and neighbour list are current: use compute coord/atom"),
    ("fix 1 all nve/mdp", "compute a all centro/atom/mdp 6 cutoff 4.0",
     "runs in the host-linked mode, where the host's atom->x and neighbour list are current: use compute centro/atom"),
    ("fix 1 all nve/mdp bricks yes", "compute a all coord/atom/mdp cutoff 25", "the cutoff 25 is beyond the pair style's cutforce"),
    ("fix 1 all nve/mdp bricks yes", "compute a all centro/atom/mdp 6 cutoff 25", "the cutoff 25 is beyond the pair style's cutforce"),
])
def test_refusals_that_need_a_run(fix, compute, msg):
    rc, out, err = _run(MOS2.replace("FIX", fix).replace("COMPUTES", compute + "\ncompute r all reduce max c_a\nthermo_style custom step c_r\n"),
                        timeout=600)
    assert rc == 1
    assert msg in err, err[-2000:]


def test_the_examples_run(tmp_path, capsys):
    """examples/in.aeam-alsi.centro-mdp.mi355x: the largest centro-symmetry parameter is above 4 A^2 at every row, the smallest
    coordination number is 11 and the mean starts at 12 - 12 / 2047; the dump of step 200 holds 12 atoms with 11 neighbours, the
    vacancy's, each above 4 A^2, while the median of the others is below 2 A^2.
    examples/in.rebomos-sheet.coord-mdp.mi355x: every Mo starts with 6 S, none ever has more, and the dumped column is the one
    the thermo reduces."""
    for f in glob.glob(os.path.join(PKG, "alsi.centro.*.dump")) + glob.glob(os.path.join(PKG, "sheet.coord.*.dump")):
        os.remove(f)
    rc, out, err = _run(script_file="examples/in.aeam-alsi.centro-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(s) for s in rows[:, 0]] == [0, 50, 100, 150, 200] and rows.shape[1] == 6
    assert np.all(rows[:, 3] > 4.0) and np.all(rows[:, 3] < 12.0) and np.all(rows[:, 4] == 11.0)
    assert rows[0, 5] == pytest.approx(12.0 - 12.0 / 2047.0, rel=PRINTED)
    _, cols, d = _read_dump(os.path.join(PKG, "alsi.centro.200.dump"))
    assert cols == "id type x y z c_cs c_nn".split() and len(d) == 2047 and sorted(glob.glob(os.path.join(PKG, "alsi.centro.*.dump")))[0].endswith("100.dump")
    eleven = np.nonzero(d[:, 6] == 11.0)[0]
    rest = np.setdiff1d(np.arange(len(d)), eleven)
    with capsys.disabled():
        print(f"alsi.centro.200.dump: {len(eleven)} atoms with 11 neighbours, centro {d[eleven, 5].min():.2f} .. {d[eleven, 5].max():.2f} A^2; the rest: median "
              f"{np.median(d[rest, 5]):.2f}, 99th percentile {np.percentile(d[rest, 5], 99):.2f}, max {d[rest, 5].max():.2f} A^2 "
              f"(types of the {int((d[rest, 5] > 4.0).sum())} above 4: {sorted(set(d[rest][d[rest, 5] > 4.0][:, 1].astype(int)))})")
    assert len(eleven) == 12 and np.all(d[eleven, 5] > 4.0) and np.median(d[rest, 5]) < 2.0
    rc, out, err = _run(script_file="examples/in.rebomos-sheet.coord-mdp.mi355x", timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    with capsys.disabled():
        print(f"sheet: c_nSmin {rows[:, 4].tolist()}, c_nSave {rows[:, 5].tolist()}")
    assert len(rows) == 11 and rows[0, 4] == 6.0 and rows[0, 5] == 6.0 and np.all(rows[:, 4] <= 6.0) and np.all(rows[:, 5] > 5.0)
    files = sorted(glob.glob(os.path.join(PKG, "sheet.coord.*.dump")), key=lambda p: int(p.split(".")[-2]))
    assert [int(p.split(".")[-2]) for p in files] == [250, 500, 750, 1000]
    _, cols, d = _read_dump(files[-1])
    assert cols == "id x y z c_nS".split() and len(d) == 576 and d[:, 4].mean() == pytest.approx(rows[-1, 5], rel=PRINTED)
