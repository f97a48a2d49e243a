"""GPU: the device FIRE minimiser (csrc/fire.hip, mdp_fire_*) against its NumPy definition (tests/fireref.py).

FIRE amplifies force differences -- near the minimum the mixing step normalises forces that are mostly noise -- so the
arithmetic of the kernels is pinned by REPLAY: every iteration of the device is repeated by ONE fireref iteration from
the device's own downloaded state and forces.  Free runs against fireref with ORACLE forces are short (120 iterations),
and convergence is judged by the oracle on the downloaded positions, not by the device's own numbers."""
import numpy as np
import pytest

from lammps_plugins_amd.host import capi, system as S
from firerig import BIG, DT, Rig, cell as _cell, replay
import fireref

pytestmark = pytest.mark.gpu

def _replay(rig, niter, need_negatives, results, modify=None):
    """firerig.replay with the bounds of this module: decisions, dt and alpha exact; dtv, s1, s2, x and v to 1e-13"""
    s = rig.s
    r = replay(rig, niter, modify=modify)
    print(f"replay {rig.style} {s.n} atoms, {niter} iterations: P <= 0 at {r['negatives']}, dt grew {r['grown']} times, dmax "
          f"shortened dtv {r['limited']} times, skipped {r['skipped']}, worst x {r['x']:.3g} A, v {r['v']:.3g} rel, "
          f"dtv/s1/s2 {r['ctl']:.3g} rel")
    assert not r["exact"], r["exact"]
    assert r["ctl"] < 1e-13, r["ctl"]
    assert r["x"] < 1e-13 and r["v"] < 1e-13, (r["x"], r["v"])
    assert r["skipped"] <= niter // 100
    assert len([n for n in r["negatives"] if n > 1]) >= need_negatives, r["negatives"]
    assert r["grown"] >= 1
    results.update(negatives=r["negatives"], limited=r["limited"])


@pytest.mark.parametrize("style,niter,need", [("rebomos", 130, 3), ("aeam", 200, 1)])
def test_every_iteration_replays_in_fireref(style, niter, need, oracle, capsys):
    """Measured on an MI355X: worst x 1.8e-15 / 3.6e-15 A, v 5.9e-16 / 1.3e-15 relative per atom,
    dtv, s1, s2 3.1e-16 / 4.3e-16 relative (REBO-MoS / AEAM; all bounds 1e-13); P <= 0 at iterations 1, 26, 67, 102, 105 and
    1, 168; no iteration skipped; dmax shortens dtv in neither window (the next test replays one where it does)."""
    rig = Rig(style, _cell(style), oracle)
    res = {}
    try:
        rig.ctx.fire_setup(0.0, 0.0, BIG, BIG)
        _replay(rig, niter, need, res)
    finally:
        rig.close()
    with capsys.disabled():
        print(capsys.readouterr().out, end="")


def test_replay_covers_a_step_shortened_by_dmax(oracle, capsys):
    """the hot strained cell (initial force norm of some 470 eV/A): dmax shortens dtv in its first iterations"""
    rig = Rig("rebomos", _cell("rebomos", hot=True), oracle)
    res = {}
    try:
        rig.ctx.fire_setup(0.0, 0.0, BIG, BIG)
        _replay(rig, 40, 0, res)
    finally:
        rig.close()
    with capsys.disabled():
        print(capsys.readouterr().out, end="")
    assert res["limited"] >= 1


def _free_run_device(rig, niter):
    """niter iterations one at a time (a state read after each); returns the P <= 0 iterations and x, v by tag"""
    negatives = []
    for it in range(1, niter + 1):
        assert rig.ctx.fire_iterate(1) == 0
        if not rig.ctx.fire_state()["mixed"]:
            negatives.append(it)
    return negatives, rig.by_tag(("x", "v"))


def _reference_run(rig, etol, ftol, maxiter, maxeval):
    x0 = S.wrap(rig.s.box, rig.s.x)
    eng = rig.engine(x0)

    def fe(x):
        o = eng.compute(x, eflag=1, vflag=0)
        return o["f_owned"], o["eng"]
    return fireref.minimize(fe, x0, rig.m, DT, S.FTM2V, etol, ftol, maxiter, maxeval)


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_free_run_of_120_iterations_follows_fireref_with_oracle_forces(style, oracle, capsys):
    """xtol = 1e-8 A is what tests/test_gpu_trajectory.py allows against the same oracle loop, and what a force difference
    at the project's 1e-9 eV/A tolerance can grow to in 120 FIRE iterations (2.1e-9 / 9.6e-9 A in a CPU experiment).
    Measured: 2.3e-13 A (REBO-MoS), 2.1e-13 .. 4.3e-13 A (AEAM, three runs), so the test asks 1e-10 A.  Then (REBO-MoS) the same 120 iterations queued in one call on a fresh context must
    give bitwise the same positions -- fixed-order sums, and a state read that leaves no trace; AEAM's three-body forces
    use float atomics, so there the two runs are compared to the replay's tolerance scaled by the iterations.  Last, the
    MD path after mdp_fire_off: 50 NVE steps from the minimiser's state equal 50 steps of a fresh context set up from
    the downloaded positions and velocities to 1e-10 A (measured 1.1e-14 A)."""
    s = _cell(style)
    rig = Rig(style, s, oracle)
    try:
        rig.ctx.fire_setup(0.0, 0.0, BIG, BIG)
        negatives, a = _free_run_device(rig, 120)
        ref = _reference_run(rig, 0.0, 0.0, 120, BIG)
        assert negatives == ref["negatives"], (negatives, ref["negatives"])
        worst = np.abs(rig.unwrap(a["x"] - ref["x"])).max()
        # the MD path afterwards
        rig.ctx.fire_off()
        for _ in range(50):
            rig.d.step(0, 0, rebuild="auto", defer_final=True)
        after = rig.by_tag(("x",))["x"]
    finally:
        rig.close()
    s2 = S.System(s.box, S.wrap(s.box, a["x"]), s.type, s.tag, s.mass)
    rig2 = Rig(style, s2, oracle, v0=a["v"])
    try:
        rig2.d.compute(0, 0)
        for _ in range(50):
            rig2.d.step(0, 0, rebuild="auto", defer_final=True)
        worst_md = np.abs(rig2.unwrap(rig2.by_tag(("x",))["x"] - after)).max()
    finally:
        rig2.close()
    rig3 = Rig(style, s, oracle)
    try:
        rig3.ctx.fire_setup(0.0, 0.0, BIG, BIG)
        rig3.ctx.fire_iterate(120)
        st = rig3.ctx.fire_state()
        b = rig3.by_tag(("x", "v"))
    finally:
        rig3.close()
    twin = np.abs(rig3.unwrap(b["x"] - a["x"])).max()
    with capsys.disabled():
        print(f"free run {style}: worst |x - x_ref| after 120 iterations {worst:.3g} A; 50 NVE steps afterwards against a "
              f"fresh context {worst_md:.3g} A; one call against 120 calls {twin:.3g} A")
    assert st["iterations"] == 120 and st["stop"] == 0
    assert worst < 1e-10, worst          # (the issue's bound is 1e-8; measured 2.3e-13 / 2.1e-13 A)
    assert worst_md < 1e-10, worst_md
    if style == "rebomos":
        assert np.array_equal(b["x"], a["x"]) and np.array_equal(b["v"], a["v"])
    else:
        assert twin < 1e-10, twin        # (measured 3.3e-13 A)


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_converges_as_judged_by_the_oracle_and_stays_latched(style, oracle, capsys):
    """ftol = 1e-6, maxiter = 4000.  The oracle's force norm on the downloaded positions is below ftol + sqrt(3N) 1e-9 and
    its energy within 1e-8 eV per atom of the reference run's final energy (fireref with oracle forces).  The iteration
    count is not compared for equality (force noise of 1e-9 eV/A changes it by tens of per cent); the cap is twice the
    reference's.  Then the latch: 50 more iterations asked for change nothing, and a run queued 64 iterations at a time
    (the host sees the stop code late and queues some too many) ends in bitwise the state of a run queued one iteration
    at a time with a wait after each (REBO-MoS only: AEAM's three-body forces use float atomics, and FIRE turns their last
    bits into another iteration count).  Measured: REBO-MoS 618 iterations (reference 618), AEAM 556, 557, 564 in three
    runs (reference 565); oracle force norm 9.8e-7 / 9.5e-7 .. 9.96e-7; oracle energy within 1e-10 eV of the reference run's."""
    ftol = 1e-6
    rig = Rig(style, _cell(style), oracle)
    try:
        st = rig.d.minimize(0.0, ftol, 4000, 100000)
        a = rig.by_tag()
        # the latch, through the C calls: set up again would restart, so use the raw calls on a second rig below; here the
        # domain-level result
        o = rig.engine(S.wrap(rig.s.box, a["x"])).compute(S.wrap(rig.s.box, a["x"]), eflag=1, vflag=0)
        ref = _reference_run(rig, 0.0, ftol, 4000, 100000)
    finally:
        rig.close()
    fn = float(np.sqrt((o["f_owned"] ** 2).sum()))
    with capsys.disabled():
        print(f"converge {style}: device {st['iterations']} iterations (reference {ref['iterations']}), oracle |f| {fn:.3g}, "
              f"device |f| {st['fnorm']:.3g}, E {o['eng']:.10f} (device {st['e_final']:.10f}, reference {ref['e_final']:.10f}), "
              f"E initial {st['e_initial']:.6f}")
    assert st["stop"] == 1 and st["criterion"] == "force tolerance"
    assert ref["stop"] == fireref.FTOL
    assert fn < ftol + np.sqrt(3 * rig.s.n) * 1e-9, fn
    assert abs(o["eng"] - ref["e_final"]) / rig.s.n < 1e-8
    assert abs(st["e_final"] - o["eng"]) / rig.s.n < 1e-9
    assert st["iterations"] <= 2 * ref["iterations"]
    assert st["evaluations"] == st["iterations"]

    rig = Rig(style, _cell(style), oracle)
    try:
        ctx = rig.ctx
        ctx.fire_setup(0.0, ftol, 4000, 100000)
        n = 0
        while not ctx.fire_iterate(1):       # (no state read in between: its energy compute would give the lists another history)
            ctx.sync()
            n += 1
            assert n <= 4001
        st1 = ctx.fire_state()
        b = rig.by_tag()
        assert ctx.fire_iterate(50) == 1
        st2 = ctx.fire_state()
        c = rig.by_tag()
    finally:
        rig.close()
    assert st1["stop"] == 1 and st1["iterations"] <= 2 * ref["iterations"]
    assert st2 == st1
    assert np.array_equal(c["x"], b["x"]) and np.array_equal(c["v"], b["v"])
    if style == "rebomos":   # (AEAM's float atomics change the count from run to run: 557 and 564 in two runs here)
        assert st1["iterations"] == st["iterations"]
        assert np.array_equal(rig.unwrap(b["x"] - a["x"]), np.zeros_like(b["x"])) and np.array_equal(b["v"], a["v"])


@pytest.mark.parametrize("which", ["maxiter", "maxeval"])
def test_the_counts_stop_at_exactly_37(which, oracle):
    rig = Rig("rebomos", _cell("rebomos"), oracle)
    try:
        kw = dict(maxiter=37, maxeval=BIG) if which == "maxiter" else dict(maxiter=BIG, maxeval=37)
        rig.ctx.fire_setup(0.0, 0.0, kw["maxiter"], kw["maxeval"])
        stop = 0
        for _ in range(4):
            stop = stop or rig.ctx.fire_iterate(25)
        st = rig.ctx.fire_state()
        a = rig.by_tag(("x",))
        rig.ctx.fire_off()
    finally:
        rig.close()
    assert st["stop"] == (3 if which == "maxiter" else 4) and stop in (0, st["stop"])
    assert st["iterations"] == 37 and st["evaluations"] == 37
    # and it is the state of iteration 37: the same run stopped by hand
    rig = Rig("rebomos", _cell("rebomos"), oracle)
    try:
        rig.ctx.fire_setup(0.0, 0.0, BIG, BIG)
        for _ in range(37):
            rig.ctx.fire_iterate(1)
            rig.ctx.sync()
        b = rig.by_tag(("x",))
    finally:
        rig.close()
    assert np.array_equal(a["x"], b["x"])


STRETCHED = dict(dmax=0.3, dtgrow=1.3, tmax=20.0)


@pytest.mark.parametrize("style,modify", [("rebomos", {}), ("aeam", {}), ("rebomos", STRETCHED)],
                         ids=["rebomos", "aeam", "rebomos-dmax0.3-dtgrow1.3-tmax20"])
def test_no_pair_is_missed_while_atoms_move(style, modify, oracle, monkeypatch, capsys):
    """Hot cells (jitter 0.3 A; REBO-MoS strained by 1.12 with an inner skin of 0.5 A): 400 iterations, and every 50 the
    device's forces against the oracle's on the device's own positions, the oracle's lists built anew each time.  The
    third case repeats it with dmax 0.3, dtgrow 1.3, tmax 20: the settings that stretch most what the advance kernel
    predicts an atom can move before the next displacement check (dmax, dtgrow and dtmax enter that prediction).
    Measured on an MI355X: worst |f - f_oracle| 4.6e-12 / 1.3e-13 / 3.6e-12 eV/A, atoms moved up to 1.45 / 0.83 / 1.34 A,
    3 / 5 / 4 reneighbourings, none late."""
    if style == "rebomos":
        monkeypatch.setenv("MDP_INNER_SKIN", "0.5")
    s = _cell(style, hot=True)
    rig = Rig(style, s, oracle)
    worst, far = 0.0, 0.0
    try:
        ctx = rig.ctx
        ctx.fire_setup(0.0, 0.0, BIG, BIG, **modify)
        x0 = rig.by_tag(("x",))["x"]
        for block in range(8):
            ctx.fire_iterate(50)
            a = rig.by_tag(("x", "f"))
            x = S.wrap(s.box, a["x"])
            o = rig.engine(x).compute(x, eflag=0, vflag=0)
            worst = max(worst, float(np.abs(o["f_owned"] - a["f"]).max()))
            far = max(far, float(np.sqrt((rig.unwrap(a["x"] - x0) ** 2).sum(axis=1)).max()))
        st = ctx.fire_state()
        builds, prunes = ctx.md_neighbor_stats()[7], ctx.md_prune_stats()
    finally:
        rig.close()
    with capsys.disabled():
        print(f"hot {style} {s.n} atoms: worst |f - f_oracle| {worst:.3g} eV/A, atoms moved up to {far:.3g} A, "
              f"{st['reneighbors']} reneighbourings, style builds / angular centres {builds}, prunings {prunes}, "
              f"E {st['e_initial']:.3f} -> {st['e_final']:.3f}")
    assert st["iterations"] == 400
    assert worst < 1e-9, worst
    assert st["e_final"] < st["e_initial"]
    assert prunes["late"] == 0 and st["late"] == 0
    if style == "rebomos":
        assert builds >= 2            # the first build and at least one the displacement trigger asked for
    else:
        assert st["reneighbors"] >= 1


def test_the_fire_suite_skips_at_most_one_iteration_in_100():
    """the `fire` net (tests/nets.py) does not replay an iteration with |cos(v, f)| < 1e-9; a case may skip one (its own
    limit), the suite's cases together at most 1 in 100 -- a condition on the suite, so it is summed here over all of it"""
    import nets
    specs = [s for seed, n in nets.SUITE["fire"] for s in nets.cases("fire", seed, n)]
    for s in specs:      # (the cases tests/test_gpu_nets.py has run in this process are not run again)
        if (s["id"], s["seed"]) not in nets.FIRE_SKIPPED:
            nets.run_fire(s)
    skipped = sum(nets.FIRE_SKIPPED[s["id"], s["seed"]] for s in specs)
    assert skipped * 100 <= sum(s["niter"] for s in specs), skipped


def test_energy_tolerance_stops_on_the_energies_of_the_computes(oracle):
    """etol > 0: every compute tallies the energy, the control kernel reads it on the device.  The stop is LAMMPS' test on
    the last two energies, more than delaystep iterations after the last P <= 0, and the energies are the oracle's."""
    etol = 1e-10
    rig = Rig("rebomos", _cell("rebomos"), oracle)
    try:
        st = rig.d.minimize(etol, 0.0, 4000, 100000)
        x = S.wrap(rig.s.box, rig.by_tag(("x",))["x"])
        o = rig.engine(x).compute(x, eflag=1, vflag=0)
        ref = _reference_run(rig, etol, 0.0, 4000, 100000)
    finally:
        rig.close()
    assert st["stop"] == 2 and st["criterion"] == "energy tolerance" and ref["stop"] == fireref.ETOL
    assert st["iterations"] - st["last_negative"] > 20
    assert abs(st["e_final"] - st["e_previous"]) < etol * 0.5 * (abs(st["e_final"]) + abs(st["e_previous"]) + 1e-8)
    assert st["e_final"] != st["e_previous"] or st["fnorm"] < 1e-3
    assert abs(st["e_final"] - o["eng"]) / rig.s.n < 1e-9
    assert abs(st["e_initial"] - ref["e_initial"]) / rig.s.n < 1e-9
    assert st["iterations"] <= 2 * ref["iterations"]
    # (two consecutive energies agree to etol well before the forces are small: the count is the reference's or near it)
    assert abs(o["eng"] - ref["e_final"]) / rig.s.n < 1e-6


def test_refusals(oracle):
    rig = Rig("rebomos", _cell("rebomos"), oracle)
    try:
        ctx = rig.ctx
        with pytest.raises(capi.MdpError, match="mdp_fire_setup not called"):
            ctx.fire_iterate(1)
        rig.d.thermostat(300.0, 300.0, 0.1)
        with pytest.raises(capi.MdpError, match="thermostat"):
            ctx.fire_setup(0.0, 1e-6, 10, 10)
        rig.d.thermostat_off()
        with pytest.raises(capi.MdpError, match="ftol"):
            ctx.fire_setup(0.0, -1.0, 10, 10)
        ctx.fire_setup(0.0, 1e-6, 10, 10)
        with pytest.raises(capi.MdpError, match="mdp_fire_off first"):
            rig.d.thermostat(300.0, 300.0, 0.1)
        with pytest.raises(capi.MdpError, match="mdp_fire_off first"):
            rig.d.langevin(300.0, 300.0, 0.1, 7)
        with pytest.raises(capi.MdpError, match="one rank only"):
            ctx.dd_setup(rig.s.box, (2, 1, 1), 0, 10.0)
        ctx.fire_off()
    finally:
        rig.close()
