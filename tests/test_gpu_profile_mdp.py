"""GPU: binned mass, momentum and kinetic energy on the device (mdp_profile_*, csrc/profile.hip; DeviceDomain.profile /
profile_read) against tests/profileref.py on positions and velocities downloaded by tag from the SAME device state.  The
device forms the fractional coordinate with fused multiply-adds, so every comparison asks the reference for n_edge == 0 (no
atom within 1e-9 of a bin edge; it fails loudly otherwise); then the counts are exact and every sum lies within
count 2^-e + 2^-50 sum|t| of the exact one (profileref.check_sums).  The states are thermal and the bin counts do not divide
the lattices, so no plane of atoms sits at an edge."""
import numpy as np
import pytest

from conftest import POT_AEAM
from lammps_plugins_amd.host import capi, resident, system as S
import profileref
from test_gpu_rdf_mdp import _by_tag, _context, _mig_system, _system, MIG_READS, MIG_RENB, MIG_STEPS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6                     # MDP_EINVAL, MDP_ESTATE of include/mdpair_hip.h
GRIDS = [((2,), (7,)), ((0, 1), (5, 11)), ((0, 1, 2), (3, 4, 5)), ((0, 1, 2), (16, 16, 16))]   # the last: 4096 rows, straight to global
PER = (True, True, True)


def _state(d, s):
    """(lam, mass, v) by tag of the device's current atoms"""
    got = d.ctx.md_download(d.nlocal, want=("x", "v"))
    tags = d.tags_local
    return s.box.x2lamda(_by_tag(s.n, tags, got["x"])), s.mass[s.type], _by_tag(s.n, tags, got["v"])


def _check(d, s, dims, nbins, periodic=PER, member=None, state=None):
    count, sums, ex = d.profile_read()
    assert count.dtype == sums.dtype == np.int64 and sums.shape == (int(np.prod(nbins)), 5)
    lam, mass, v = _state(d, s) if state is None else state
    ref = profileref.table(lam, periodic, dims, nbins, mass, v, exponents=ex, member=member)
    # the exponents are the rule applied to the global range of the members' terms
    assert ex.tolist() == [capi.profile_exponent(r, s.n) for r in ref["rng"]] == [profileref.exponent(r, s.n) for r in ref["rng"]]
    return count, sums, ex, ref, profileref.check_sums(count, sums, ex, ref)


@pytest.mark.parametrize("temp", [300.0, 2500.0])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_brick(style, temp, capsys):
    """25 steps (the device's own displacement check decides the rebuilds), the last with its final half deferred; every grid
    against the reference, two reads identical, and the kinetic-energy column summed over the bins equal to md_thermo's"""
    s, v0 = _system(style, temp)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.compute(0, 0)
        for k in range(25):
            d.step(0, 0, rebuild="auto", defer_final=k == 24)
        worst = {}
        for n, (dims, nbins) in enumerate(GRIDS):
            d.profile(dims, nbins)
            if n == 0:                       # read right after the step whose final half was deferred
                count, sums, ex = d.profile_read()
                ke = d.thermo()["ke"]
                mv2 = float(np.ldexp(sums[:, 4].astype(np.float64), -int(ex[4])).sum())
                assert abs(mv2 - 2.0 * ke / S.MVV2E) <= 1e-12 * mv2 and mv2 > 0.0, (mv2, 2.0 * ke / S.MVV2E)
            count, sums, ex, ref, worst[nbins] = _check(d, s, dims, nbins)
            again = d.profile_read()
            assert all(np.array_equal(a, b) for a, b in zip((count, sums, ex), again))
            assert count.sum() == s.n and ctx.profile_info()["rows"] == count.size and ctx.profile_info()["ndim"] == len(dims)
            assert (count > 0).sum() > min(count.size, s.n) // 4          # the atoms spread over the bins
            # the first column is the mass: the same in every bin per atom, so its quantised sum is exact to count units
            arr = resident.profile_normalise(count, sums, ex, nbins, s.box.volume, S.BOLTZ, S.MVV2E, 1.0 / 0.602214129, False)
            want = profileref.normalise(count, sums, ex, nbins, s.box.volume, S.BOLTZ, S.MVV2E, 1.0 / 0.602214129, False)
            assert np.allclose(arr, want, rtol=1e-13, atol=1e-13)
            tmean = (arr[:, len(dims)] * arr[:, len(dims) + 3]).sum() / s.n
            assert abs(tmean - 2.0 * ke / (3.0 * s.n * S.BOLTZ)) <= 1e-9 * tmean
        with capsys.disabled():
            print(f"{style} {temp:.0f} K: {d.builds} list builds, worst error / bound per grid "
                  + ", ".join(f"{'x'.join(map(str, k))}: {w:.3f}" for k, w in worst.items()))
    finally:
        ctx.close()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_group(style):
    """the mask of `type 1, or above the mid-plane`: counts and sums over the members only; a group bit without a mask is
    refused"""
    s, v0 = _system(style, 300.0)
    member = (s.type == 1) | (s.x[:, 2] > s.box.lo[2] + 0.5 * s.box.prd[2])
    assert 0.5 * s.n < member.sum() < s.n
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        with pytest.raises(capi.MdpError, match="no mask covers the current atoms") as e:
            ctx.profile_setup([0], [5], group_bit=2)
        assert e.value.code == ESTATE
        mask = np.ones(s.n + 1, dtype=np.int32)
        mask[1:] |= 2 * member.astype(np.int32)
        d.set_group(mask, 1)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        for dims, nbins in GRIDS[1:]:
            d.profile(dims, nbins, group_bit=2)
            count, sums, ex, ref, _ = _check(d, s, dims, nbins, member=member)
            assert count.sum() == member.sum()
        d.profile((2,), (7,))
        assert d.profile_read()[0].sum() == s.n
        d.profile((2,), (7,), group_bit=2)
        ctx.md_set_mask(None)                # the mask withdrawn under a measurement that needs it
        for read in (ctx.profile_range, lambda: ctx.profile_sums([0] * 5)):
            with pytest.raises(capi.MdpError, match="no mask covers the current atoms") as e:
                read()
            assert e.value.code == ESTATE
    finally:
        ctx.close()


def _bricks_run(s, v0, world, grids, steps=0, reads=(0,), renb=0):
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            out = {}
            if steps:
                d.compute(0, 0)
            for step in range(0, steps + 1):
                if step:
                    d.step(0, 0, rebuild=step % renb == 0)
                if step in reads:
                    got = ctx.md_download(d.nlocal, want=("x", "v"))
                    out[step] = dict(tags=d.tags_local.copy(), x=got["x"], v=got["v"], tables=[])
                    for dims, nbins in grids:
                        d.profile(dims, nbins)
                        out[step]["tables"].append(d.profile_read())
            return out
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    merged = {}
    for step in reads:
        got = [r[step]["tables"] for r in res]
        assert all(np.array_equal(a, b) for g in got for ta, tb in zip(g, got[0]) for a, b in zip(ta, tb))   # every rank reads the same
        x, v, owner, seen = np.zeros((s.n, 3)), np.zeros((s.n, 3)), np.zeros(s.n, dtype=int), np.zeros(s.n, dtype=int)
        for k, r in enumerate(res):
            o = r[step]
            x[o["tags"] - 1], v[o["tags"] - 1], owner[o["tags"] - 1] = o["x"], o["v"], k
            seen[o["tags"] - 1] += 1
        assert np.all(seen == 1)
        merged[step] = dict(tables=got[0], x=x, v=v, owner=owner)
    return merged


def test_bricks_exact():
    """the (2, 2, 2) MoS2 replica with thermal velocities, no step taken: on 1, 2 and 8 bricks the exponents, the counts and
    the sums are identical integers"""
    s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 2))
    v0 = S.gaussian_velocities(s, 300.0, seed=8)
    runs = {w: _bricks_run(s, v0, w, GRIDS)[0] for w in (1, 2, 8)}
    for w in (2, 8):
        assert len(set(runs[w]["owner"])) == w
        for (count, sums, ex), (count1, sums1, ex1) in zip(runs[w]["tables"], runs[1]["tables"]):
            assert np.array_equal(ex, ex1) and np.array_equal(count, count1) and np.array_equal(sums, sums1)
    for (count, sums, ex), (dims, nbins) in zip(runs[1]["tables"], GRIDS):
        assert count.sum() == s.n and count.size == np.prod(nbins) and np.array_equal(sums[:, 0] > 0, count > 0)
        assert np.abs(sums[:, 4]).max() > 2 ** 40                          # the headroom is used: these are not small integers


def test_bricks_migrating(capsys):
    """the drift of tests/test_gpu_rdf_mdp.py (40 steps, reneighbourings every 5) on 8 bricks: the rank-summed tables at
    steps 20 and 40 against the reference on the gathered state, and atoms changed owner between the reads"""
    s, v0 = _mig_system()
    grids = [GRIDS[1], GRIDS[3]]
    run = _bricks_run(s, v0, 8, grids, steps=MIG_STEPS, reads=MIG_READS, renb=MIG_RENB)
    for step in MIG_READS:
        lam, mass = s.box.x2lamda(run[step]["x"]), s.mass[s.type]
        for (count, sums, ex), (dims, nbins) in zip(run[step]["tables"], grids):
            ref = profileref.table(lam, PER, dims, nbins, mass, run[step]["v"], exponents=ex)
            assert ex.tolist() == [profileref.exponent(r, s.n) for r in ref["rng"]]
            worst = profileref.check_sums(count, sums, ex, ref)
            assert count.sum() == s.n
            with capsys.disabled():
                print(f"8 bricks, step {step}, {'x'.join(map(str, nbins))}: worst error / bound {worst:.3f}")
    moved = int((run[MIG_READS[0]]["owner"] != run[MIG_READS[-1]]["owner"]).sum())
    assert len(set(run[MIG_READS[-1]]["owner"])) == 8 and moved >= 3, moved


def test_a_non_periodic_dimension():
    """the alloy with free z at 2 500 K: atoms leave the box in z and are counted in the edge bins"""
    s, v0 = _system("aeam", 2500.0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, nonperiodic=(0, 0, 1))
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        per = (True, True, False)
        state = _state(d, s)
        below, above = int((state[0][:, 2] < 0.0).sum()), int((state[0][:, 2] >= 1.0).sum())
        assert below > 5 and above >= 0 and below + above < s.n // 4, (below, above)
        for dims, nbins in (((2,), (7,)), ((0, 2), (5, 7))):
            d.profile(dims, nbins)
            count, sums, ex, ref, _ = _check(d, s, dims, nbins, periodic=per, state=state)
            assert count.sum() == s.n
        wrapped = profileref.table(state[0], PER, (2,), (7,), state[1], state[2])["count"]
        d.profile((2,), (7,))
        count = d.profile_read()[0]
        assert count[0] - wrapped[0] == below - above and not np.array_equal(count, wrapped)      # clamped, not wrapped
    finally:
        ctx.close()


def test_refusals():
    s = S.rebomos_bulk_cell()
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=S.gaussian_velocities(s, 300.0, seed=4))
        assert ctx.profile_info() == dict(on=False, rows=0, ndim=0, serial=0)
        for read in (ctx.profile_range, lambda: ctx.profile_sums([0] * 5)):
            with pytest.raises(capi.MdpError, match="mdp_profile_setup not called") as e:
                read()
            assert e.value.code == ESTATE
        bad = [
            (([], []), "ndim must be 1 .. 3, not 0"),
            (([0, 1, 2, 0], [2, 2, 2, 2]), "ndim must be 1 .. 3, not 4"),
            (([0, 0], [2, 2]), "dimension 0 is named twice"),
            (([2, 1, 2], [2, 2, 2]), "dimension 2 is named twice"),
            (([3], [2]), "dimension 3 is not 0, 1 or 2"),
            (([-1], [2]), "dimension -1 is not 0, 1 or 2"),
            (([0], [0]), "nbin must be >= 1, not 0"),
            (([0, 1], [4, -4]), "nbin must be >= 1, not -4"),
            (([0], [capi.PROFILE_MAXBINS + 1]), "more than 1048576 rows"),
            (([0, 1], [1024, 1025]), "more than 1048576 rows"),
            (([0, 1, 2], [2 ** 30, 2 ** 30, 8]), "more than 1048576 rows"),
        ]
        for (dims, nbins), text in bad:
            with pytest.raises(capi.MdpError, match=text) as e:
                ctx.profile_setup(dims, nbins)
            assert e.value.code == EINVAL, (dims, nbins, e.value.code)
        assert not ctx.profile_info()["on"]
        ctx.profile_setup([0, 1], [1024, 1024])                                  # the cap itself is accepted, and read
        first = ctx.profile_info()
        count, sums = ctx.profile_sums([capi.profile_exponent(r, s.n) for r in ctx.profile_range()])
        assert count.sum() == s.n and count.size == capi.PROFILE_MAXBINS
        ctx.profile_setup([2], [7])                                              # a second setup replaces the first
        second = ctx.profile_info()
        assert first["on"] and second["serial"] > first["serial"] and (second["rows"], second["ndim"]) == (7, 1)
        rng = ctx.profile_range()
        assert np.all(rng > 0.0)
        ex = [capi.profile_exponent(r, s.n) for r in rng]
        assert ctx.profile_sums(ex)[0].sum() == s.n
        for k, name in enumerate(["m", "m vx", "m vy", "m vz", r"m v\^2"]):      # an exponent too large, column by column
            big = list(ex)
            big[k] += (s.n - 1).bit_length() + 1                                 # the term with the range now reaches 2^62 / n
            with pytest.raises(capi.MdpError, match=rf"column {k} \({name}\)") as e:
                ctx.profile_sums(big)
            assert e.value.code == EINVAL
        assert ctx.profile_sums(ex)[0].sum() == s.n                              # and the next read is clean
        ctx.profile_off()
        assert not ctx.profile_info()["on"]
        with pytest.raises(capi.MdpError, match="mdp_profile_setup not called") as e:
            ctx.profile_range()
        assert e.value.code == ESTATE and d.nlocal == s.n
    finally:
        ctx.close()
    # without mdp_dd_setup, and without mdp_md_setup
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        with pytest.raises(capi.MdpError, match="mdp_md_setup not called") as e:
            ctx.profile_setup([0], [5])
        assert e.value.code == ESTATE
        cfg = capi.MdConfig()
        cfg.style, cfg.nlocal, cfg.nghost, cfg.ntypes = st, s.n, 0, 2
        cfg.skin, cfg.dt, cfg.ftm2v, cfg.mvv2e, cfg.nghost_self = skin, 0.001, S.FTM2V, S.MVV2E, 0
        for k in range(3):
            cfg.bbox_lo[k], cfg.bbox_hi[k] = -30.0, 60.0
        e3, e1 = np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
        ctx.md_setup(cfg, s.x, np.zeros_like(s.x), s.type, s.tag, s.mass, map_, e1, e3, e1, e1)
        for call in (lambda: ctx.profile_setup([0], [5]), ctx.profile_range, lambda: ctx.profile_sums([0] * 5)):
            with pytest.raises(capi.MdpError, match="mdp_dd_setup not called") as e:
                call()
            assert e.value.code == ESTATE
    finally:
        ctx.close()


# ---- the slots the small systems above leave empty: more than 256 blocks and a workgroup that walks many of them
# (MDP_MEASURE_GRID), the two sides of the LDS / global switch, a box with all three tilts, a group of nobody, 0 K, bit 31
BIG_GRIDS = [((2,), (7,)), ((0,), (819,)), ((0, 1, 2), (16, 16, 16))]


@pytest.fixture(scope="module")
def big():
    """70 304 aluminium atoms (fcc 26^3, as the indenter's second-trip test), jittered by 0.05 A so that no lattice plane sits
    at a bin edge, at 300 K; built once for this module"""
    s = S.fcc_cell(4.045, 26)
    s.mass[1:3] = capi.AeamFile(POT_AEAM).mass[:2]
    s = S.jitter(s, 0.05, seed=61)
    assert s.n == 70304 and -(-s.n // 256) == 275
    return s, S.gaussian_velocities(s, 300.0, seed=62)


def test_many_blocks_and_one_workgroup_read_the_same(big, monkeypatch, capsys):
    """275 blocks: unset, profile_range_total_kernel strides over more than 256 slots; at MDP_MEASURE_GRID = 3 and 1 every
    kernel's loop takes 92 and 275 trips and, at 1, one workgroup flushes everything.  The range, the exponents and the
    tables of a 7-row, an 819-row (the largest LDS layout) and a 4 096-row grid (straight to global) are identical under the
    three settings, and inside check_sums' bound of the reference.  No step is taken.  The atom the device keeps last (the
    positions alone decide the order; a first set-up tells which it is) is given the largest velocity components of all, so
    the maxima of the momentum and energy columns come from slot 274, beyond the first trip over the slots."""
    s, v0 = big
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        last = int(resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0).tags_local[-1])
    finally:
        ctx.close()
    v0 = v0.copy()
    v0[last - 1] = 1.5 * np.abs(v0).max(axis=0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        assert d.nlocal == s.n and -(-d.nlocal // 256) > 256           # the premise: the slot loop takes a second trip
        assert int(d.tags_local[-1]) == last
        state = _state(d, s)
        assert all(int(np.argmax(np.abs(profileref.terms(state[1], state[2])[:, k]))) == last - 1 for k in range(1, 5))
        got = {}
        for knob in (None, "3", "1"):
            if knob is None:
                monkeypatch.delenv("MDP_MEASURE_GRID", raising=False)
            else:
                monkeypatch.setenv("MDP_MEASURE_GRID", knob)
            got[knob] = []
            for dims, nbins in BIG_GRIDS:
                d.profile(dims, nbins)
                got[knob].append((ctx.profile_range(),) + d.profile_read())
        monkeypatch.delenv("MDP_MEASURE_GRID", raising=False)
        t = profileref.terms(state[1], state[2])
        # a maximum, whatever the grid: m and m v are one product each, the same bits in NumPy; m v.v is formed with fused
        # multiply-adds on the device, within 3 roundings of NumPy's
        tmax = np.abs(t).max(axis=0)
        rng = got[None][0][0]
        assert np.array_equal(rng[:4], tmax[:4]) and abs(rng[4] - tmax[4]) <= 4 * 2.0 ** -53 * tmax[4]
        worst = []
        for k, (dims, nbins) in enumerate(BIG_GRIDS):
            _, count, sums, ex = got[None][k]
            for knob in ("3", "1"):
                assert all(np.array_equal(a, b) for a, b in zip(got[knob][k], (rng, count, sums, ex))), (knob, nbins)
            ref = profileref.table(state[0], PER, dims, nbins, state[1], state[2], exponents=ex)
            assert ex.tolist() == [profileref.exponent(r, s.n) for r in ref["rng"]]
            worst.append(profileref.check_sums(count, sums, ex, ref))
            assert count.sum() == s.n and (count > 0).sum() >= min(count.size, 52)      # (52 lattice planes, 0.1 A thick, along x)
        with capsys.disabled():
            print("70 304 atoms, knob unset / 3 / 1 identical; worst error / bound per grid " + ", ".join(f"{w:.3f}" for w in worst))
    finally:
        ctx.close()


def test_either_side_of_the_lds_switch():
    """the 1 152-atom MoS2 state after 10 steps: 819 rows are the largest table a workgroup keeps in LDS (4 095 sums, then 819
    counts from byte 32 760), 820 rows go straight to global.  1-d grids of 819 and 820 bins and 3-d grids of (9, 7, 13) and
    (4, 5, 41) rows against the reference; the exponents depend on the range alone, so the 1-d pair summed over all rows
    gives the same integers, column by column"""
    s, v0 = _system("rebomos", 300.0)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        state = _state(d, s)
        got = {}
        for dims, nbins in (((0,), (819,)), ((0,), (820,)), ((0, 1, 2), (9, 7, 13)), ((0, 1, 2), (4, 5, 41))):
            rows = int(np.prod(nbins))
            assert (rows * 5 <= 4096) == (rows == 819) and rows in (819, 820)
            d.profile(dims, nbins)
            count, sums, ex, ref, _ = _check(d, s, dims, nbins, state=state)
            assert count.sum() == s.n
            got[nbins] = (count, sums, ex)
        a, b = got[(819,)], got[(820,)]
        assert np.array_equal(a[2], b[2]) and a[0].sum() == b[0].sum() and np.array_equal(a[1].sum(axis=0), b[1].sum(axis=0))
        assert np.array_equal(got[(9, 7, 13)][1].sum(axis=0), got[(4, 5, 41)][1].sum(axis=0))
    finally:
        ctx.close()


def _sheared_alloy():
    """the 864-atom alloy sheared homogeneously into the box with all three tilts of
    test_the_centre_of_mass_in_a_cell_sheared_in_xz_and_yz (tests/test_gpu_spring_mdp.py), at 300 K with a drift that takes
    atoms through the faces in x, y and z within 30 steps"""
    s0, v0 = _system("aeam", 300.0)
    box = S.Box(s0.box.lo.copy(), s0.box.prd.copy(), np.array([0.35, -0.45, 0.25]))
    s = S.System(box, np.ascontiguousarray(box.lamda2x(s0.box.x2lamda(s0.x))), s0.type, s0.tag, s0.mass)
    return s, v0 + np.array([500.0, -400.0, 300.0]), S.Box(box.lo, box.prd, np.array([0.35, 0.0, 0.0]))


def test_a_box_with_all_three_tilts():
    """dd_x2lamda's yz and xz terms: after 30 steps of the drift (the lists rebuilt every step, images changed in x, y and z)
    a profile over (z, x) and one over (x, y, z) against the reference.  Not vacuous: the reference in the box stripped of xz
    and yz counts differently"""
    s, v0, flat = _sheared_alloy()
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.track_images()
        d.compute(0, 0)
        for _ in range(30):
            d.step(0, 0, rebuild=True)
        assert all((d.images_local()[:, k] != 0).sum() > s.n // 4 for k in range(3))
        got = d.ctx.md_download(d.nlocal, want=("x", "v"))
        x, v = _by_tag(s.n, d.tags_local, got["x"]), _by_tag(s.n, d.tags_local, got["v"])
        for dims, nbins in (((2, 0), (5, 7)), ((0, 1, 2), (6, 5, 7))):
            d.profile(dims, nbins)
            count, sums, ex, ref, _ = _check(d, s, dims, nbins, state=(s.box.x2lamda(x), s.mass[s.type], v))
            other = profileref.table(flat.x2lamda(x), PER, dims, nbins, s.mass[s.type], v, exponents=ex)
            assert count.sum() == s.n and (other["count"] != ref["count"]).sum() > 10, nbins
    finally:
        ctx.close()


def test_nobody_zero_kelvin_and_bit_31():
    """a group bit no atom carries: range, exponents and tables all 0.  Velocities exactly zero: the exponents of the momentum
    and energy columns are 0 and their sums 0, the mass column and the counts exact.  A group on bit 31 (the sign bit of the
    mask) against the reference"""
    s, _ = _system("rebomos", 300.0)
    member = s.tag % 3 == 0
    mask = np.ones(s.n + 1, dtype=np.uint32)
    mask[1:][member] |= 0x80000000
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=np.zeros((s.n, 3)))
        d.set_group(mask.view(np.int32), 0)
        for dims, nbins in (((2,), (7,)), ((0, 1), (41, 20))):                  # LDS, and straight to global
            d.profile(dims, nbins, group_bit=4)
            assert not ctx.profile_range().any()
            count, sums, ex = d.profile_read()
            assert not ex.any() and not count.any() and not sums.any() and count.size == int(np.prod(nbins))
            d.profile(dims, nbins)                                              # everyone, at 0 K
            count, sums, ex, ref, _ = _check(d, s, dims, nbins)
            assert not ex[1:].any() and not sums[:, 1:].any() and ex[0] == profileref.exponent(s.mass[1:3].max(), s.n)
            assert np.array_equal(sums[:, 0], ref["sums"][:, 0]) and count.sum() == s.n
    finally:
        ctx.close()
    s, v0 = _system("rebomos", 300.0)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(mask.view(np.int32), 0)
        d.compute(0, 0)
        for _ in range(5):
            d.step(0, 0, rebuild="auto")
        for dims, nbins in (((2,), (7,)), ((0, 1), (41, 20))):
            d.profile(dims, nbins, group_bit=-2 ** 31)
            count, sums, ex, ref, _ = _check(d, s, dims, nbins, member=member)
            assert count.sum() == member.sum() == s.n // 3
    finally:
        ctx.close()
