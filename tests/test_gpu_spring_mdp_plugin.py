"""GPU: `fix spring/mdp` through `plugin load` + `run` in the mini-host, handing its settings to one `fix nve/mdp bricks yes`
(its Fix::extract("mdp_springs") block).  The shipped bilayer example cut to 300 steps: the columns of one row come from one
read and fit each other (E = f[1]^2 / 2K, f[4] = |f[1]| with R0 = 0), the pull grows as the tether point leaves, the held
sulphur plane has not moved, and the rows of steps 0 and 300 are what the library gives for the same atoms -- positions,
image flags and groups from write_dump, handed to a DeviceDomain with one spring at the step's tether point -- to the
bounds of tests/test_gpu_spring_mdp.py plus half a unit of the eighth digit the mini-host prints.  Then the refusals that
need a run."""
import os

import numpy as np
import pytest

from conftest import POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from test_plugin_boundary import PKG, _run, _thermo_rows
from test_gpu_spring_mdp import E_TOL, F_TOL

pytestmark = pytest.mark.gpu

K, X0, VX, DT = 5.0, 19.46, 2.0, 0.001


def _dump(path, ncol):
    rows = [l.split() for l in open(path).read().splitlines()[5:]]
    a = np.array([[float(w) for w in r] for r in rows])
    assert a.shape[1] == ncol, a.shape
    return a


def _library_state(all_dump, mo_ids, upper_ids, step):
    """mdp_spring_state for the atoms of a dump (id x y z vx vy vz ix iy iz), with the example's spring at `step`"""
    n = len(all_dump)
    ids = all_dump[:, 0].astype(np.int32)
    assert np.array_equal(ids, np.arange(1, n + 1))
    b = S.rebomos_bulk_cell().box
    box = S.Box(np.zeros(3), np.array([b.prd[0], b.prd[1], 41.9483041764]), b.tilt.copy()).replicate((3, 2, 1))
    typ = np.full(n, 2, dtype=np.int32)
    typ[mo_ids - 1] = 1
    s = S.System(box, np.ascontiguousarray(all_dump[:, 1:4]), typ, ids, np.array([0.0, 95.95, 32.065]))
    by_tag = np.ones(n + 1, dtype=np.int32)
    by_tag[upper_ids] |= 2
    p = capi.read_rebomos_file(POT_REBOMOS)
    ctx = capi.Context(0)
    try:
        ctx.rebomos_set_params(p)
        d = resident.DeviceDomain(ctx, capi.STYLE_REBOMOS, s, 3.0 * p.rcmax[0][0] + 1.0, 1.0, [0, 0, 1], v0=np.ascontiguousarray(all_dump[:, 4:7]))
        d.set_group(by_tag, 0)
        d.track_images(resident.image_pack(all_dump[:, 7:10].astype(np.int64)))
        d.compute(0, 0)
        d.spring([dict(k=K, r0=0.0, c=(X0 + VX * step * DT, None, None), bit=2)])
        return d.spring_state(0)
    finally:
        ctx.close()


def test_the_bilayer_example_pulls_the_upper_layer_and_prints_what_the_library_gives(tmp_path, capsys):
    text = open(os.path.join(PKG, "examples", "in.rebomos-bilayer.spring-mdp.mi355x")).read()
    cols = "id x y z vx vy vz ix iy iz"
    dumps = "".join(f"write_dump {g} custom {tmp_path / (g + '.TAG')} {cols}\n" for g in ("all", "held", "upper"))
    assert "run 2000" in text and "thermo 100\n" in text
    text = text.replace("thermo 100\n", "thermo 50\ngroup mo type 1\n" + f"write_dump mo custom {tmp_path / 'mo'} {cols}\n" + dumps.replace("TAG", "0"))
    text = text.replace("run 2000", "run 300\n" + dumps.replace("TAG", "1"))
    rc, out, err = _run(text, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(r) for r in rows[:, 0]] == list(range(0, 301, 50))
    e, fx, fmag = rows[:, 5], rows[:, 6], rows[:, 7]
    with capsys.disabled():
        print("bilayer example, f_pull[1] by step: " + " ".join(f"{int(n)}:{f:.5g}" for n, f in zip(rows[:, 0], fx)))
    # one read per row: E = K dx^2 / 2 with f[1] = -K dx, and R0 = 0 makes dr = |dx| >= 0 (eight digits are printed)
    assert np.allclose(e, fx * fx / (2.0 * K), rtol=3e-7, atol=1e-12) and np.allclose(fmag, np.abs(fx), rtol=1e-7, atol=0.0)
    assert fx[-1] > fx[0] + 1.0 and fx[-1] > 0.0                   # the tether point has left by 0.6 A: K dx gains about 3 eV/A
    held0, held1 = (tmp_path / "held.0").read_text().splitlines()[5:], (tmp_path / "held.1").read_text().splitlines()[5:]
    assert len(held0) == 288 and held0 == held1                     # the held sulphur plane: digit for digit
    mo = _dump(tmp_path / "mo", 10)[:, 0].astype(np.int64)
    for tag, step, row in (("0", 0, rows[0]), ("1", 300, rows[-1])):
        upper = _dump(tmp_path / f"upper.{tag}", 10)[:, 0].astype(np.int64)
        assert len(upper) == 864
        st = _library_state(_dump(tmp_path / f"all.{tag}", 10), mo, upper, step)
        assert st["atoms"] == 864
        for got, want, tol in ((row[5], st["energy"], E_TOL), (row[6], st["ftotal"][0], F_TOL), (row[7], st["ftotal"][3], F_TOL)):
            assert abs(got - want) <= tol + 0.5e-7 * abs(want), (step, got, want)


ALLOY = """plugin load aeamplugin.so
plugin load springmdpplugin.so
plugin load heatmdpplugin.so
plugin load nvtmdpplugin.so
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
group substrate region floor
group mobile subtract all substrate
timestep 0.001
velocity all create 300.0 1082337
velocity substrate set 0.0 0.0 0.0
fix integrate mobile nve/mdp bricks yes
thermo_style custom step temp pe ke etotal f_pull f_pull[1] f_pull[2] f_pull[3] f_pull[4]
thermo 10
"""
PULL = "fix pull mobile spring/mdp tether 5.0 22.0 NULL 20.0 1.0 vel 0.0 0.0 3.0\n"
RUN = "run 50\n"


def test_the_columns_of_a_run_on_the_alloy_and_a_second_run_starts_the_tether_again():
    rc, out, err = _run(ALLOY.replace("thermo 10\n", "thermo 50\n") + PULL + RUN + RUN, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(r) for r in rows[:, 0]] == [0, 50, 50, 100]
    assert np.all(rows[:, 5] > 0.0) and not rows[:, 7].any()                       # y is NULL
    assert np.allclose(np.sqrt((rows[:, 6:9] ** 2).sum(axis=1)), np.abs(rows[:, 9]), rtol=1e-6)
    assert rows[1, 5] != rows[2, 5]              # the row that opens the second run has the tether point back at c


@pytest.mark.parametrize("deck,msg", [
    (ALLOY.replace("fix integrate mobile nve/mdp bricks yes\n", "") + PULL, "Fix spring/mdp requires fix nve/mdp with bricks yes as the time integrator"),
    (ALLOY.replace(" bricks yes", "") + PULL,
     "Fix spring/mdp: fix integrate runs in the host-linked mode, where the host keeps atom->image itself: use fix spring (or run the fix with bricks yes)"),
    (ALLOY.replace("fix integrate mobile nve/mdp bricks yes\n", "fix integrate mobile nvt/mdp temp 300.0 300.0 0.1\n") + PULL,
     "Fix spring/mdp: fix pull cannot run next to fix integrate (nvt/mdp)"),
    (ALLOY + PULL + "fix hot mobile heat/mdp 1 0.5\n", "Fix spring/mdp: fix pull cannot run next to fix hot (heat/mdp)"),
    (ALLOY + PULL.replace("pull mobile", "pull all"), "Fix spring/mdp: group all has 1200 atoms outside group mobile of fix integrate (nve/mdp): the spring acts on atoms the integrator moves"),
], ids=["no-integrator", "host-linked", "nvt", "heat", "held-atoms"])
def test_init_refusals(deck, msg):
    rc, out, err = _run(deck.replace(" f_pull f_pull[1] f_pull[2] f_pull[3] f_pull[4]", "") + RUN, timeout=300)
    assert rc == 1
    assert msg in err, err[-2000:]


def test_a_host_side_integrator_is_refused():
    rc, out, err = _run(ALLOY.replace("fix integrate mobile nve/mdp bricks yes\n", "fix integrate mobile nve\n").replace(
        " f_pull f_pull[1] f_pull[2] f_pull[3] f_pull[4]", "") + PULL + RUN, timeout=300)
    # (under LAMMPS `fix nve` is a time_integrate fix and is named as one that integrates on the host; the mini-host's own
    # integrator is no Fix in Modify's list, so there the run misses fix nve/mdp)
    assert rc == 1 and ("integrates on the host" in err or "Fix spring/mdp requires fix nve/mdp" in err), err[-2000:]


def test_minimize_mdp_refuses_to_run_over_a_spring():
    rc, out, err = _run(ALLOY + PULL + "minimize/mdp 0.0 1.0e-4 100 1000\n", timeout=300)
    assert rc == 1
    assert "minimize/mdp: fix pull (spring/mdp) is not applied by the minimiser; unfix it first" in err, err[-2000:]


def test_two_ranks_are_refused():
    from test_gpu_minilmp_ranks import _double_env
    rc, out, err = _run(ALLOY + PULL + RUN, np=2, env=_double_env(), timeout=300)
    assert rc == 1 and "Fix spring/mdp runs on one MPI rank only" in err, err[-2000:]
