"""GPU: one moving atom at every lane.  The displacement checks vote per wave (__any / __ballot) and lane 0 stores the
answer; a vote placed inside the lane-0 branch would count one atom in 64, and a grid-stride loop that stopped early
would miss the atoms past its first pass.  Each test takes a system at rest, moves exactly ONE atom at a chosen device
slot (the order read back with tags_local) and asserts the library's own observable: silent at 0.45 h (no trigger is
below h/2), fired at 0.99 h without a "dangerous" count, fired at 1.05 h and counted wherever the route keeps a count;
h = the hard limit (half the skin).

Slots: every lane of wave 0; lanes 0, 1, 31, 32, 62, 63 of waves 1-3 of block 0 and of a later block; the last atom (a
partial wave); and at the large sizes one atom past grid cap x 256, which only the grid-stride loop reaches.

a. moved_kernel<false> (mdp_md_moved_async, grid cap 1024): resident domain, md_upload_x, the answer one call later.
b. moved_kernel of REBO-MoS (rebomos_check_launch, grid cap 2048).  Resident: md_upload_x makes the next compute check the
   style's own lists at once against half the inner skin (check_now; no rows pruned, so moved_kernel<false>); observable:
   the style-list builds of rebomos_list_info().  Host mode: set_positions_host + rebomos_compute_host with pruned rows
   active, so moved_kernel<true>; observables: the re-prunings of md_prune_stats() and the style-list builds.
c. nve_advance_kernel's CHECK vote (mdp_md_integrate_check): one atom given a velocity in a crystal at rest must cause a
   reneighboring before it reaches the hard limit (no dangerous count); none happens with its velocity zeroed.  REBO-MoS
   counts its style-list builds and row prunings too (the MdpStyleCheck votes of the same kernel), with no late one."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S

pytestmark = pytest.mark.gpu

LANES = (0, 1, 31, 32, 62, 63)


def _slots(n, later_block=2):
    out = list(range(64))
    out += [256 * 0 + 64 * w + l for w in (1, 2, 3) for l in LANES]
    out += [256 * later_block + 64 * w + l for w in (0, 1, 2, 3) for l in LANES]
    out.append(n - 1)
    return sorted({k for k in out if k < n})


def _aeam(cells):
    af = capi.AeamFile(POT_AEAM)
    tabs = af.build()
    ctx = capi.Context(0)
    ctx.aeam_set_tables(tabs)
    s = S.fcc_cell(4.045, cells)              # pure Al: a perfect crystal feels no force
    s.mass[1:3] = af.mass[:2]
    return ctx, s, float(af.cut_table(tabs).max()) + 1.0, 1.0, None


def _rebo(rep):
    p = capi.read_rebomos_file(POT_REBOMOS)
    ctx = capi.Context(0)
    ctx.rebomos_set_params(p)
    return ctx, S.replicate(S.rebomos_bulk_cell(), rep), 3.0 * p.rcmax[0][0] + 2.0, 2.0, [0, 0, 1]


def _domain(style, size, v0=None):
    ctx, s, cutghost, skin, map_ = (_aeam if style == capi.STYLE_AEAM else _rebo)(size)
    d = resident.DeviceDomain(ctx, style, s, cutghost, skin, map_, v0=np.zeros((s.n, 3)) if v0 is None else v0)
    return ctx, s, d, skin


DIRS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])


# ---------------------------------------------------------------------------------------------------------------- a.
def _moved_sweep(style, size, slots):
    ctx, s, d, skin = _domain(style, size)
    try:
        d.compute(0, 0)
        h = 0.5 * skin
        x0 = ctx.md_download(d.nlocal, want=("x",))["x"]
        ctx.md_moved_async()
        bad = []
        for j, k in enumerate(slots):
            assert k < d.nlocal
            for frac, fire, danger in ((0.45, False, False), (0.99, True, False), (1.05, True, True)):
                x = x0.copy()
                x[k] += frac * h * DIRS[j % len(DIRS)]
                ctx.md_upload_x(x)
                ctx.md_moved_async()                       # (the answer of the check launched before the upload)
                got = ctx.md_moved_async()                 # the check of the moved positions
                if got != (fire, danger):
                    bad.append((k, frac, got))
                ctx.md_upload_x(x0)
                ctx.md_moved_async()
        return bad, d.nlocal
    finally:
        ctx.close()


@pytest.mark.parametrize("style,size", [(capi.STYLE_AEAM, 6), (capi.STYLE_REBOMOS, (3, 1, 1))], ids=["aeam-864", "rebomos-864"])
def test_moved_async_sees_one_atom_at_every_lane(style, size):
    n = 4 * size ** 3 if style == capi.STYLE_AEAM else 288 * 3
    assert n % 64 and n > 3 * 256           # a partial last wave, a later block
    bad, nlocal = _moved_sweep(style, size, _slots(n))
    assert nlocal == n
    assert not bad, f"(slot, displacement / h, (moved, dangerous)) that disagree: {bad[:12]}"


def test_moved_async_sees_one_atom_in_the_grid_stride_tail():
    """41^3 fcc cells = 275 684 atoms: the check's grid is capped at 1024 blocks of 256 (262 144 atoms a pass)"""
    n = 4 * 41 ** 3
    slots = [1024 * 256 + 5, 1024 * 256 + 64 + 37, n - 1]
    bad, nlocal = _moved_sweep(capi.STYLE_AEAM, 41, slots)
    assert nlocal == n > 1024 * 256
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- b.
def _style_list_sweep(rep, slots):
    ctx, s, d, _ = _domain(capi.STYLE_REBOMOS, rep)
    try:
        d.compute(0, 0)
        x0 = ctx.md_download(d.nlocal, want=("x",))["x"]
        bad = []
        for j, k in enumerate(slots):
            assert k < d.nlocal
            # the immediate check's trigger is h itself: 0.99 h stays silent here
            for frac, fire in ((0.45, False), (0.99, False), (1.05, True)):
                h = 0.5 * ctx.md_list_state()["skin"]      # (adaptive: a trigger that fires often widens it)
                assert 0.1 < h < 2.0
                x = x0.copy()
                x[k] += frac * h * DIRS[j % len(DIRS)]
                b0 = ctx.rebomos_list_info()["builds"]
                ctx.md_upload_x(x)
                d.compute(0, 0)
                if (ctx.rebomos_list_info()["builds"] > b0) != fire:
                    bad.append((k, frac))
                ctx.md_upload_x(x0)
                d.compute(0, 0)
        late = ctx.md_list_state()["late_builds"]
        return bad, late, d.nlocal, d.nlocal + d.nghost
    finally:
        ctx.close()


def test_style_lists_see_one_atom_at_every_lane():
    bad, late, nlocal, _ = _style_list_sweep((3, 1, 1), _slots(864))
    assert nlocal == 864
    assert not bad, f"(slot, displacement / h) whose style-list build disagrees: {bad[:12]}"
    assert late == 0


def test_style_lists_see_one_atom_in_the_grid_stride_tail():
    """13 x 13 x 11 MoS2 cells = 535 392 owned atoms: the style's check is capped at 2048 blocks of 256 (524 288 atoms a
    pass, owned atoms first)"""
    slots = [2048 * 256 + 3, 2048 * 256 + 128 + 33]
    bad, late, nlocal, nall = _style_list_sweep((13, 13, 11), slots)
    assert nlocal > 2048 * 256 + 200 and nall > nlocal
    assert not bad and late == 0, bad


def _host_prune_sweep(monkeypatch, rep, slots):
    """REBO-MoS in host mode (the plain plugin path): atoms uploaded once, then set_positions_host + rebomos_compute_host
    with one atom moved.  Host mode runs moved_kernel<true> before every compute: the style's own lists against half the
    inner skin and the pruned rows against half the pruning buffer (flag[2]: re-prune).  The knobs fix both widths here
    (they adapt otherwise) and keep the host's order on the device (no spatial sort), so host index = device slot."""
    monkeypatch.setenv("MDP_HOST_SORT", "0")
    monkeypatch.setenv("MDP_INNER_SKIN", "1.0")
    monkeypatch.setenv("MDP_PRUNE_BUFFER", "0.5")
    monkeypatch.delenv("MDP_PRUNE", raising=False)
    p = capi.read_rebomos_file(POT_REBOMOS)
    s = S.replicate(S.rebomos_bulk_cell(), rep)
    x0, type_all, tag_all, owner, shift, nloc, _ = S.with_ghosts(s, 3.0 * p.rcmax[0][0] + 2.0)
    ctx = capi.Context(0)
    try:
        ctx.rebomos_set_params(p)
        ctx.set_atoms_host(nloc, x0, type_all, tag_all, 2, map_=[0, 0, 1])
        ctx.set_skin(2.0)
        ctx.rebomos_compute_host(nloc, eflag=0, vflag=0)
        ctx.rebomos_compute_host(nloc, eflag=0, vflag=0)
        pr = ctx.md_prune_stats()
        assert pr["active"] and pr["buffer"] == pytest.approx(0.5)
        hp, hl = 0.25, 0.5                  # half the pruning buffer, half the inner skin
        bad = []
        for j, k in enumerate(slots):
            assert k < nloc
            # (prune trigger: half the buffer less a margin, never below a quarter of it; list trigger: h itself)
            for d, prune, build in ((0.45 * hp, False, False), (1.05 * hp, True, False), (0.99 * hl, True, False),
                                    (1.05 * hl, True, True)):
                x = x0.copy()
                x[k] += d * DIRS[j % len(DIRS)]
                x[nloc:] = x[owner] + shift         # the host's ghosts move with their owners
                p0, b0 = ctx.md_prune_stats()["prunings"], ctx.rebomos_list_info()["builds"]
                ctx.set_positions_host(x)
                ctx.rebomos_compute_host(nloc, eflag=0, vflag=0)
                got = (ctx.md_prune_stats()["prunings"] > p0, ctx.rebomos_list_info()["builds"] > b0)
                if got != (prune, build):
                    bad.append((k, round(d / hl, 3), got))
                ctx.set_positions_host(x0)
                ctx.rebomos_compute_host(nloc, eflag=0, vflag=0)
        return bad, ctx.md_prune_stats()["late"], nloc, len(x0)
    finally:
        ctx.close()


def test_host_mode_pruned_rows_and_style_lists_see_one_atom_at_every_lane(monkeypatch):
    bad, late, nloc, _ = _host_prune_sweep(monkeypatch, (3, 1, 1), _slots(864))
    assert nloc == 864
    assert not bad, f"(slot, displacement / h, (re-pruned, lists rebuilt)) that disagree: {bad[:12]}"
    assert late == 0


def test_host_mode_pruned_rows_see_one_atom_in_the_grid_stride_tail(monkeypatch):
    """535 392 owned atoms: the check's grid is capped at 2048 blocks of 256 (524 288 atoms a pass)"""
    bad, late, nloc, nall = _host_prune_sweep(monkeypatch, (13, 13, 11), [2048 * 256 + 3, 2048 * 256 + 128 + 33])
    assert nloc > 2048 * 256 + 200 and nall > nloc
    assert not bad and late == 0, bad


# ---------------------------------------------------------------------------------------------------------------- c.
def _events(ctx, d):
    """reneighborings; for REBO-MoS also the builds of the style's own lists and the prunings of its rows"""
    if d.style == capi.STYLE_AEAM:
        return d.builds
    return d.builds + ctx.rebomos_list_info()["builds"] + ctx.md_prune_stats()["prunings"]


def _projectile(style, size, slot, speed, steps):
    """(events, dangerous, distance flown, late) of a run with ONE atom at `speed` A/ps"""
    ctx, s, d, skin = _domain(style, size)
    tag = int(d.tags_local[slot])
    ctx.close()
    v0 = np.zeros((s.n, 3))
    v0[np.nonzero(s.tag == tag)[0][0]] = speed * np.array([0.48, 0.6, 0.64])
    ctx, s, d, skin = _domain(style, size, v0=v0)
    try:
        assert int(d.tags_local[slot]) == tag
        d.compute(0, 0)
        x0 = ctx.md_download(d.nlocal, want=("x",))["x"][slot]
        d.step(0, 0, rebuild="auto")
        b0 = _events(ctx, d)                  # (after the setup's own reneighboring, list build and first pruning)
        for _ in range(steps - 1):
            d.step(0, 0, rebuild="auto")
        x1 = ctx.md_download(d.nlocal, want=("x",))["x"]
        i = int(np.nonzero(d.tags_local == tag)[0][0])
        far = float(np.linalg.norm(x1[i] - x0))
        late = ctx.md_prune_stats()["late"] + ctx.md_list_state()["late_builds"]
        return _events(ctx, d) - b0, d.dangerous, far, late
    finally:
        ctx.close()


@pytest.mark.parametrize("style,size", [(capi.STYLE_AEAM, 6), (capi.STYLE_REBOMOS, (3, 1, 1))], ids=["aeam-864", "rebomos-864"])
def test_integrate_check_sees_one_moving_atom_at_every_lane(style, size):
    """30 A/ps: 0.03 A a step, past h (0.5 / 1.0 A) well within the run; the deferred answer must come in time.

    The alloy takes the full slot list: pure Al at rest feels no force, so the projectile flies and a slot is judged
    whenever it got past 0.8 h (most must).  REBO-MoS takes a shorter list (lanes 0, 1, 31, 33, 62, 63 of wave 0, one slot
    of wave 1, one of a later block, the last atom): the lattice stops the atom within about h, so the run shows the
    style's own votes (list builds, re-prunings) rather than the host-level CHECK vote, and each slot costs two
    55-step runs.  The REBO-MoS style votes are swept at every lane by the site-b tests above."""
    skin = 1.0 if style == capi.STYLE_AEAM else 2.0
    steps = 30 if style == capi.STYLE_AEAM else 55
    slots = _slots(864) if style == capi.STYLE_AEAM else [0, 1, 31, 33, 62, 63, 64 + 31, 256 * 2 + 64 * 3 + 62, 863]
    h = 0.5 * skin
    # the same run with the atom's velocity zeroed: no reneighboring (REBO-MoS may still re-prune its rows on its own)
    ctrl, dangerous, far, late = _projectile(style, size, slots[-1], 0.0, steps)
    assert dangerous == 0 and late == 0 and far < 0.1 * h
    assert ctrl == 0 if style == capi.STYLE_AEAM else ctrl <= 1
    bad, flown = [], 0
    for k in slots:
        events, dangerous, far, late = _projectile(style, size, k, 30.0, steps)
        flown += far > h
        # (an atom the lattice stopped short of the trigger needs no reneighboring; REBO-MoS atoms always re-prune)
        if (events <= ctrl and (far > 0.8 * h or style == capi.STYLE_REBOMOS)) or dangerous or late:
            bad.append((k, events, dangerous, round(far, 3), late))
    assert not bad, f"(slot, events, dangerous, distance flown, late): {bad[:12]}"
    if style == capi.STYLE_AEAM:
        assert flown >= len(slots) // 2     # most projectiles did fly past h (REBO-MoS: the lattice stops them sooner)
