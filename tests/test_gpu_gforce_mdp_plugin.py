"""GPU: `fix setforce/mdp`, `fix addforce/mdp` and `fix aveforce/mdp` through `plugin load` + `run` in the mini-host, handing
their settings to one `fix nve/mdp` (its Fix::extract("mdp_gforces") block), in both of its modes where the style allows.
The two shipped examples cut to 100 steps: the thermo columns f_ID[k] of steps 0 and 100 are what the library gives for the
same atoms -- positions, velocities, image flags and groups from write_dump, handed to a DeviceDomain with the same slots --
to the bounds of tests/test_gpu_gforce_mdp.py plus half a unit of the eighth digit the mini-host prints; the gripped atoms
have kept their velocity digit for digit and the held ones have not moved; and without the thermostat the atoms of step 100
are those of the library-direct run of the same set-up from the atoms of step 0.  Then the refusals that need a run, and
f_ID across two runs."""
import os

import numpy as np
import pytest

from conftest import POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
from test_plugin_boundary import PKG, _run, _thermo_rows
from gforceref import F_TOL
from test_gpu_gforce_mdp import XTOL, VTOL

pytestmark = pytest.mark.gpu

NRUN = 100
COLS = "id x y z vx vy vz ix iy iz"
DECKS = {
    # example, replicate, groups dumped, the slots of the library-direct run (bit = 4 << index of the group), thermo columns
    # as (slot, component)
    "tensile": ("in.rebomos-ribbon.tensile-mdp.mi355x", (2, 3, 1), ("held", "grip"),
                lambda bit: [dict(kind="set", f=(0.0, 0.0, 0.0), bit=bit["grip"])], ((0, 0), (0, 1))),
    "load": ("in.rebomos-bilayer.load-mdp.mi355x", (3, 2, 1), ("held", "top"),
             lambda bit: [dict(kind="set", f=(0.0, 0.0, None), bit=bit["top"]), dict(kind="ave", f=(None, None, -0.05), bit=bit["top"])],
             ((0, 0), (1, 2))),
}


def _dump(path):
    rows = [l.split() for l in open(path).read().splitlines()[5:]]
    a = np.array([[float(w) for w in r] for r in rows])
    assert a.shape[1] == 10, a.shape
    return a


def _deck(name, tmp_path, bricks, thermostat):
    example, rep, groups, slots, cols = DECKS[name]
    text = open(os.path.join(PKG, "examples", example)).read()
    assert "run 2000" in text and "thermo 100\n" in text and "fix integrate mobile nve/mdp bricks yes\n" in text
    dumps = "".join(f"write_dump {g} custom {tmp_path / (g + '.TAG')} {COLS}\n" for g in ("all",) + groups)
    text = text.replace("thermo 100\n", "thermo 50\ngroup mo type 1\n" + f"write_dump mo custom {tmp_path / 'mo'} {COLS}\n" + dumps.replace("TAG", "0"))
    text = text.replace("run 2000", f"run {NRUN}\n" + dumps.replace("TAG", "1"))
    if not bricks:
        text = text.replace("nve/mdp bricks yes", "nve/mdp")
    if not thermostat:
        lines = [l for l in text.splitlines() if not l.startswith("fix warm ")]
        assert len(lines) == len(text.splitlines()) - 1
        text = "\n".join(lines) + "\n"
    return text


def _library(name, tmp_path, tag, nsteps=0):
    """the slots of the deck on the atoms of the dump `tag`, library-direct: ([state of slot k] for the forces of those atoms,
    and after nsteps steps x, v by id)"""
    example, rep, groups, slots, cols = DECKS[name]
    a = _dump(tmp_path / f"all.{tag}")
    n = len(a)
    ids = a[:, 0].astype(np.int32)
    assert np.array_equal(ids, np.arange(1, n + 1))
    b = S.rebomos_bulk_cell().box
    box = S.Box(np.zeros(3), np.array([b.prd[0], b.prd[1], 41.9483041764]), b.tilt.copy()).replicate(rep)
    typ = np.full(n, 2, dtype=np.int32)
    typ[_dump(tmp_path / "mo")[:, 0].astype(np.int64) - 1] = 1
    s = S.System(box, np.ascontiguousarray(a[:, 1:4]), typ, ids, np.array([0.0, 95.95, 32.065]))
    by_tag = np.ones(n + 1, dtype=np.int32)
    bit = {}
    for k, g in enumerate(groups):
        bit[g] = 4 << k
        by_tag[_dump(tmp_path / f"{g}.{tag}")[:, 0].astype(np.int64)] |= bit[g]
    by_tag[1:] |= np.where(by_tag[1:] & bit["held"], 0, 2)          # mobile: everything but the held atoms
    p = capi.read_rebomos_file(POT_REBOMOS)
    ctx = capi.Context(0)
    try:
        ctx.rebomos_set_params(p)
        d = resident.DeviceDomain(ctx, capi.STYLE_REBOMOS, s, 3.0 * p.rcmax[0][0] + 1.0, 1.0, [0, 0, 1], v0=np.ascontiguousarray(a[:, 4:7]))
        d.set_group(by_tag, 2)
        d.track_images(resident.image_pack(a[:, 7:10].astype(np.int64)))
        d.compute(0, 0)
        sl = slots(bit)
        d.gforce(sl)
        states = [d.gforce_state(k) for k in range(len(sl))]
        for _ in range(nsteps):
            d.step(0, 0, rebuild="auto", defer_final=True)
        d.flush()
        got = ctx.md_download(d.nlocal, want=("x", "v"))
        x, v = np.zeros((n, 3)), np.zeros((n, 3))
        x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
        return states, x, v, box
    finally:
        ctx.close()


@pytest.mark.parametrize("bricks", [True, False], ids=["bricks", "host-linked"])
@pytest.mark.parametrize("name", ["tensile", "load"])
def test_the_examples_print_what_the_library_gives(tmp_path, name, bricks, capsys):
    example, rep, groups, slots, cols = DECKS[name]
    rc, out, err = _run(_deck(name, tmp_path, bricks, True), timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(r) for r in rows[:, 0]] == list(range(0, NRUN + 1, 50))
    with capsys.disabled():
        print(f"{name} example ({'bricks' if bricks else 'host-linked'}), columns 6 and 7 by step: " +
              " ".join(f"{int(r[0])}:{r[5]:.5g},{r[6]:.5g}" for r in rows))
    held0, held1 = (tmp_path / "held.0").read_text().splitlines()[5:], (tmp_path / "held.1").read_text().splitlines()[5:]
    assert len(held0) > 0 and held0 == held1                        # the held atoms: digit for digit
    for tag, row in (("0", rows[0]), ("1", rows[-1])):
        states = _library(name, tmp_path, tag)[0]
        for col, (k, c) in zip((5, 6), cols):
            want = states[k]["ftotal"][c]
            assert abs(row[col] - want) <= F_TOL + 0.5e-7 * abs(want), (name, tag, col, row[col], want)
    acted = groups[1]
    a0, a1 = _dump(tmp_path / f"{acted}.0"), _dump(tmp_path / f"{acted}.1")
    assert len(a0) == len(a1) > 0 and np.array_equal(a0[:, 0], a1[:, 0])
    b = S.rebomos_bulk_cell().box
    box = S.Box(np.zeros(3), np.array([b.prd[0], b.prd[1], 41.9483041764]), b.tilt.copy()).replicate(rep)
    moved = a1[:, 1:4] + S.mul_upper(a1[:, 7:10] - a0[:, 7:10], box.h) - a0[:, 1:4]      # (unwrapped: a remap may have taken a box vector off)
    if name == "tensile":           # setforce 0 0 0: the grip keeps its velocity digit for digit and has moved on at it
        assert np.array_equal(a0[:, 4:7], a1[:, 4:7]) and np.all(a0[:, 5] == 0.5)
        assert np.abs(moved - a0[:, 4:7] * (NRUN * 0.001)).max() < 1e-11
        assert abs(rows[-1][6]) > abs(rows[0][6])                    # the ribbon pulls back
    else:                           # setforce 0 0 NULL + aveforce: the plane stays where it is laterally and moves along z as one
        assert np.abs(moved[:, :2]).max() < 1e-12 and not a1[:, 4:6].any()
        assert np.ptp(a1[:, 6]) < 1e-12 and a1[0, 6] != 0.0
        assert np.ptp(moved[:, 2]) < 1e-12


@pytest.mark.parametrize("bricks", [True, False], ids=["bricks", "host-linked"])
@pytest.mark.parametrize("name", ["tensile", "load"])
def test_the_final_atoms_are_those_of_the_library_direct_run(tmp_path, name, bricks, capsys):
    """without the thermostat (its random numbers are the mini-host's to seed): 100 steps from the atoms of step 0"""
    rc, out, err = _run(_deck(name, tmp_path, bricks, False), timeout=600)
    assert rc == 0, err[-3000:]
    states, x, v, box = _library(name, tmp_path, "0", nsteps=NRUN)
    a1 = _dump(tmp_path / "all.1")
    dx = a1[:, 1:4] - x
    dx -= np.round(box.x2lamda(dx + box.lo)) @ box.h.T
    wx, wv = float(np.abs(dx).max()), float(np.abs(a1[:, 4:7] - v).max())
    with capsys.disabled():
        print(f"{name} ({'bricks' if bricks else 'host-linked'}) against the library-direct run: |dx| {wx:.2e} A, |dv| {wv:.2e} A/ps after {NRUN} steps")
    assert wx < XTOL and wv < VTOL, (wx, wv)


ALLOY = """plugin load aeamplugin.so
plugin load gforcemdpplugin.so
plugin load heatmdpplugin.so
plugin load nvtmdpplugin.so
plugin load minimizemdpplugin.so
plugin load indentmdpplugin.so
plugin load springmdpplugin.so
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
region roof block 0 10 0 10 7.9 10
group substrate region floor
group mobile subtract all substrate
group lid region roof
timestep 0.001
velocity all create 300.0 1082337
velocity substrate set 0.0 0.0 0.0
fix integrate mobile nve/mdp bricks yes
thermo_style custom step temp pe ke etotal
thermo 10
"""
GRIP = "fix grip lid setforce/mdp 0.0 0.0 NULL\n"
LOAD = "fix load lid aveforce/mdp NULL NULL -0.01\n"
BODY = "fix body mobile addforce/mdp 0.0 0.0 -0.001\n"
TIP = "fix tip mobile indent/mdp 20.0 sphere 20.0 20.0 44.0 6.0 units box\n"
PULL = "fix pull lid spring/mdp tether 5.0 NULL NULL 40.0 0.0\n"
WARM = "fix warm mobile langevin/mdp 300.0 300.0 0.1 48271\n"
RUN = "run 50\n"
NLID = 800      # four planes of 200 atoms


@pytest.mark.parametrize("deck,msg", [
    (ALLOY.replace("fix integrate mobile nve/mdp bricks yes\n", "") + GRIP, "Fix setforce/mdp requires fix nve/mdp as the time integrator"),
    (ALLOY.replace(" bricks yes", "") + BODY,
     "Fix addforce/mdp: fix integrate runs in the host-linked mode, where the host keeps atom->image itself: use fix addforce (or run the fix with bricks yes)"),
    (ALLOY.replace("fix integrate mobile nve/mdp bricks yes\n", "fix integrate mobile nvt/mdp temp 300.0 300.0 0.1\n") + GRIP,
     "Fix setforce/mdp: fix grip cannot run next to fix integrate (nvt/mdp)"),
    (ALLOY + LOAD + "fix hot mobile heat/mdp 1 0.5\n", "Fix aveforce/mdp: fix load cannot run next to fix hot (heat/mdp)"),
    (ALLOY + GRIP.replace("grip lid", "grip all"),
     "Fix setforce/mdp: group all has 1200 atoms outside group mobile of fix integrate (nve/mdp): the force acts on atoms the integrator moves"),
    (ALLOY + LOAD + GRIP, f"Fix setforce/mdp: fixes load (aveforce/mdp) and grip share {NLID} atoms (groups lid and lid); a fix defined after an "
                          "aveforce/mdp must not share atoms with it: define grip first"),
    (ALLOY + LOAD + BODY, f"Fix addforce/mdp: fixes load (aveforce/mdp) and body share {NLID} atoms (groups lid and mobile)"),
    (ALLOY + GRIP + TIP, f"Fix setforce/mdp: grip is defined before fix tip (indent/mdp), which shares {NLID} atoms with it; the device applies "
                         "setforce/mdp behind indent/mdp: define tip first, then grip"),
    (ALLOY + LOAD + PULL, f"Fix aveforce/mdp: load is defined before fix pull (spring/mdp), which shares {NLID} atoms with it; the device applies "
                          "aveforce/mdp behind spring/mdp: define pull first, then load"),
    (ALLOY + WARM + GRIP, f"Fix setforce/mdp: grip is defined after fix warm (langevin/mdp), which shares {NLID} atoms with it; the device applies "
                          "setforce/mdp in front of langevin/mdp: define grip first, then warm"),
], ids=["no-integrator", "add-host-linked", "nvt", "heat", "held-atoms", "behind-ave", "add-behind-ave", "indent-after", "spring-after", "langevin-before"])
def test_init_refusals(deck, msg):
    rc, out, err = _run(deck + RUN, timeout=300)
    assert rc == 1
    assert msg in err, err[-2000:]


def test_the_orders_the_device_reproduces_run_and_f_id_carries_across_two_runs():
    """the indenter and the spring defined first, the thermostat last; addforce stands anywhere.  Between two runs f_ID holds
    the last read; the row that opens the second run is read anew from the same atoms"""
    cols = " f_grip[1] f_grip[3] f_load[3] f_body f_body[3]"
    deck = ALLOY.replace("thermo_style custom step temp pe ke etotal", "thermo_style custom step temp pe ke etotal" + cols).replace("thermo 10\n", "thermo 50\n")
    rc, out, err = _run(deck + BODY + TIP + PULL + GRIP + LOAD + WARM + RUN + RUN, timeout=600)
    assert rc == 0, err[-3000:]
    rows = np.array(_thermo_rows(out))
    assert [int(r) for r in rows[:, 0]] == [0, 50, 50, 100]
    assert np.all(rows[:, 5] != 0.0) and np.all(rows[:, 8] != 0.0)
    # setforce left z alone, so the aveforce behind it finds the same z total: one read per row serves both
    assert np.array_equal(rows[:, 6], rows[:, 7])
    # the second run opens on the atoms the first one left: the same forces, computed again
    assert np.allclose(rows[2, 5:10], rows[1, 5:10], rtol=1e-6, atol=1e-6)


def test_a_host_side_integrator_is_refused():
    rc, out, err = _run(ALLOY.replace("fix integrate mobile nve/mdp bricks yes\n", "fix integrate mobile nve\n") + GRIP + RUN, timeout=300)
    # (under LAMMPS `fix nve` is a time_integrate fix and is named as one that integrates on the host; the mini-host's own
    # integrator is no Fix in Modify's list, so there the run misses fix nve/mdp)
    assert rc == 1 and ("integrates on the host" in err or "Fix setforce/mdp requires fix nve/mdp" in err), err[-2000:]


@pytest.mark.parametrize("fix,style", [(GRIP, "grip (setforce/mdp)"), (BODY, "body (addforce/mdp)"), (LOAD, "load (aveforce/mdp)")])
def test_minimize_mdp_refuses_to_run_over_the_family(fix, style):
    rc, out, err = _run(ALLOY + fix + "minimize/mdp 0.0 1.0e-4 100 1000\n", timeout=300)
    assert rc == 1
    assert f"minimize/mdp: fix {style} is not applied by the minimiser; unfix it first" in err, err[-2000:]


def test_two_ranks_are_refused():
    from test_gpu_minilmp_ranks import _double_env
    rc, out, err = _run(ALLOY + GRIP + RUN, np=2, env=_double_env(), timeout=300)
    assert rc == 1 and "Fix setforce/mdp runs on one MPI rank only" in err, err[-2000:]
