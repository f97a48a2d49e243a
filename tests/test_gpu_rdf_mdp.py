"""GPU: pair-distance histograms on the device (mdp_rdf_*, csrc/rdf.hip; DeviceDomain.rdf / rdf_read) against tests/rdfref.py,
the NumPy brute force, on positions downloaded by tag from the SAME device state.  The device compiles with
-ffp-contract=fast and forms ghost positions as x + shift, so the last bit of r may differ from NumPy's and nothing else:
a device histogram is right when hist_sure <= device <= hist_sure + edge_adjacent for every column and bin (rdfref), and
every test caps the reference's edge pairs at 2 (expected: below 1e-2 for 1e5 - 1e6 pairs and a window of 2e-9 of a bin).
All states are thermal: lattice distances at 0 K would sit where rounding decides."""
import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
import nets
import rdfref

pytestmark = pytest.mark.gpu

PER = (1, 1, 1)
NBIN = 50
EINVAL, ESTATE = -1, -6                     # MDP_EINVAL, MDP_ESTATE of include/mdpair_hip.h
PAIRS = [((1, 2), (1, 2)), (1, 1), (1, 2), (2, 1), (2, 2)]                 # * *, 1 1, 1 2, 2 1, 2 2
RANGES = [(1, 2, 1, 2), (1, 1, 1, 1), (1, 1, 2, 2), (2, 2, 1, 1), (2, 2, 2, 2)]


def _context(style):
    ctx = capi.Context(0)
    if style == "rebomos":
        p = capi.read_rebomos_file(POT_REBOMOS)
        ctx.rebomos_set_params(p)
        return ctx, capi.STYLE_REBOMOS, 2.0, 3.0 * p.rcmax[0][0] + 2.0, [0, 0, 1]
    af = capi.AeamFile(POT_AEAM)
    tabs = af.build()
    ctx.aeam_set_tables(tabs)
    return ctx, capi.STYLE_AEAM, 1.0, float(af.cut_table(tabs).max()) + 1.0, None


def _system(style, temp, seed=3, frac_si=0.05):
    """the 1 152-atom MoS2 cell in its sheared box / the 864-atom fcc alloy with 5 % of type 2, at temp"""
    if style == "rebomos":
        s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
    else:
        s = S.fcc_cell(4.045, 6, frac_type2=frac_si, seed=92)
        s.mass[1:3] = capi.AeamFile(POT_AEAM).mass[:2]
    return s, S.gaussian_velocities(s, temp, seed=seed)


def _by_tag(n, tags, a):
    out = np.zeros((n,) + a.shape[1:], dtype=a.dtype)
    out[tags - 1] = a
    return out


def _x_by_tag(d, n):
    return _by_tag(n, d.tags_local, d.ctx.md_download(d.nlocal, want=("x",))["x"])


@pytest.mark.parametrize("temp", [300.0, 2500.0])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_brick(style, temp, capsys):
    """25 steps with no forced rebuild (the device's own displacement check decides), so the read happens with ghosts as old
    as the run leaves them; 50 bins, the cutoff at its limit cutghost - skin, the columns * *, 1 1, 1 2, 2 1, 2 2.  The
    device histogram inside the reference's bracket, icount / jcount / dup exact, two reads identical, and the first-shell
    bins occupied.  Not vacuous: the histogram holds more than 1e5 entries -- pair-column entries, summed over the five
    columns, so each pair of the * * column is there twice (* * is the sum of the other four) -- and the * * column alone
    more than 5e4 pairs: 864 alloy atoms with the 78 neighbours fcc has inside 6.5 A are 6.7e4 at the most, less what the
    thermal spread of the outermost shell (6.40 A) puts beyond the cutoff -- all that system can hold at the cutoff
    limit; the 1 152-atom MoS2 cell holds 3e5."""
    s, v0 = _system(style, temp)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        cutoff = cutghost - skin
        d.rdf(NBIN, cutoff, PAIRS)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        hist, ic, jc, du = d.rdf_read()
        again = d.rdf_read()
        assert all(np.array_equal(a, b) for a, b in zip((hist, ic, jc, du), again))
        assert hist.dtype == np.int64 and hist.shape == (5, NBIN)
        ref = rdfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, cutoff, NBIN, RANGES)
        with capsys.disabled():
            print(f"{style} {temp:.0f} K: cutoff {cutoff:.4f} A, {d.builds} list builds, {int(hist[0].sum())} pairs in * *, {int(hist.sum())} in all, "
                  f"{ref['n_edge']} edge pairs, device - reference {int(np.abs(hist - ref['hist']).sum())} counts")
        rdfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"]) and np.array_equal(jc, ref["jcount"]) and np.array_equal(du, ref["dup"])
        n1, n2 = int((s.type == 1).sum()), int((s.type == 2).sum())
        assert ic.tolist() == [s.n, n1, n1, n2, n2] and du.tolist() == [s.n, n1, 0, 0, n2] and n2 > 0
        assert hist.sum() > 1e5 and hist[0].sum() > 5e4
        assert np.array_equal(hist[0], hist[1:].sum(axis=0)) and hist[2].sum() == hist[3].sum() > 0
        first = 2.41 if style == "rebomos" else 4.045 / np.sqrt(2.0)       # Mo-S bond / fcc nearest neighbours
        b0 = int(first * NBIN / cutoff)
        assert hist[0][b0 - 1:b0 + 2].sum() > s.n and hist[0][:b0 // 2].sum() == 0
        arr = resident.rdf_normalise(hist, ic, jc, du, cutoff, s.box.volume)
        assert np.allclose(arr, rdfref.normalise(hist, ic, jc, du, cutoff, s.box.volume), rtol=1e-13, atol=1e-13)
    finally:
        ctx.close()


# ---- the slots test_one_brick leaves empty: 8 192 counters and column 32, one bin, cells widened by bin_grid's cap, a
# workgroup that walks many chunks (MDP_MEASURE_GRID), a free dimension
FIVE = (3, 2)                  # the alloy relabelled to 3 metal and 2 angular types
TYPE_RANGES = [(lo, hi) for lo in range(1, 6) for hi in range(lo, 6)]                    # the 15 inclusive ranges over 5 types
# 32 of their 120 unordered pairs (a column and its transpose hold the same histogram)
RANGES32 = [a + b for k, a in enumerate(TYPE_RANGES) for b in TYPE_RANGES[k:]][::3][:32]
SMALL_CUTOFF = {"rebomos": 2.8, "aeam": 3.0}     # above the first shells (2.41, 2.86 A); test_a_small_cutoff asserts what they are for
_FIVE = {}


def _five_types(temp=300.0):
    """the 864-atom alloy with 30 % Si relabelled to 5 types as nets.run_aeam_types relabels it: (s, v0, af, tabs)"""
    import os
    import tempfile
    import aeam_five
    if not _FIVE:
        nmet, nang = FIVE
        path = os.path.join(tempfile.mkdtemp(), "five.aeam")
        aeam_five.write_relabelled_file(path, POT_AEAM, [0] * nmet + [1] * nang, ["M%d" % i for i in range(nmet)] + ["X%d" % i for i in range(nang)])
        af = capi.AeamFile(path)
        s2 = S.fcc_cell(4.045, 6, frac_type2=0.3, seed=92)
        r = np.random.default_rng(5)
        ty = np.where(s2.type == 1, r.integers(1, nmet + 1, s2.n), r.integers(nmet + 1, nmet + nang + 1, s2.n)).astype(np.int32)
        _FIVE.update(af=af, tabs=af.build(), s=S.System(s2.box, s2.x.copy(), ty, s2.tag.copy(), np.array([0.0] + list(af.mass))))
    s = _FIVE["s"]
    return s, S.gaussian_velocities(s, temp, seed=3), _FIVE["af"], _FIVE["tabs"]


def _five_context():
    s, v0, af, tabs = _five_types()
    ctx = capi.Context(0)
    ctx.aeam_set_tables(tabs)
    return ctx, capi.STYLE_AEAM, 1.0, float(af.cut_table(tabs).max()) + 1.0, None


def _nall(ctx):
    info = ctx.dd_info()
    return info["nlocal"] + info["nself"] + info["nrecv"]


def test_8192_counters_and_column_32(capsys):
    """32 columns x 256 bins, all the LDS histogram holds, on the alloy relabelled to 5 types: 32 pairwise different pairs
    of type ranges, so that no column can stand in for another; column 32 (mask bit 31) is not empty and is not column 31"""
    s, v0, af, tabs = _five_types()
    assert len(set(RANGES32)) == 32 and len(np.unique(s.type)) == 5
    ctx, st, skin, cutghost, map_ = _five_context()
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        cutoff = cutghost - skin
        d.rdf(256, cutoff, [((r[0], r[1]), (r[2], r[3])) for r in RANGES32])
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        hist, ic, jc, du = d.rdf_read()
        assert hist.shape == (32, 256) and ctx.rdf_info()["nbin"] * ctx.rdf_info()["npair"] == 8192
        ref = rdfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, cutoff, 256, RANGES32)
        with capsys.disabled():
            print(f"{int(hist.sum())} entries, column 32: {int(hist[31].sum())}, {ref['n_edge']} edge pairs")
        rdfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"]) and np.array_equal(jc, ref["jcount"]) and np.array_equal(du, ref["dup"])
        assert ref["hist_sure"][31].sum() > 1000 and not np.array_equal(ref["hist"][31], ref["hist"][30])
        assert all(ref["hist_sure"][m].sum() > 0 for m in range(32))
        assert len({ref["hist"][m].tobytes() for m in range(32)}) == 32            # the columns are pairwise different in what they hold, too
    finally:
        ctx.close()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_bin(style):
    """nbin = 1: the one counter of a column is the number of its pairs inside the cutoff -- the reference's, and the sum of
    the 50 bins read on the same state"""
    s, v0 = _system(style, 300.0)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        cutoff = 0.8 * (cutghost - skin)
        d.compute(0, 0)
        for _ in range(5):
            d.step(0, 0, rebuild="auto")
        d.rdf(1, cutoff, PAIRS)
        one = d.rdf_read()
        d.rdf(NBIN, cutoff, PAIRS)
        many = d.rdf_read()
        ref = rdfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, cutoff, 1, RANGES)
        rdfref.check_bracket(one[0], ref)
        assert one[0].shape == (5, 1) and one[0][0, 0] > 1e4 and all(np.array_equal(a, b) for a, b in zip(one[1:], many[1:]))
        if ref["n_edge"] == 0:      # (no pair within 1e-9 of the cutoff itself: the two reads then hold the same pairs)
            assert np.array_equal(one[0][:, 0], many[0].sum(axis=1)) and np.array_equal(one[0], ref["hist"])
    finally:
        ctx.close()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_a_small_cutoff_widens_the_cells(style, capsys):
    """A cutoff just above the first shell: cells of cutoff / 2 over the brick's bounding box would be more than bin_grid's
    cap of 4 nall + 4096 (the premise, asserted from nets.measure_bin_grid over the box the domain sets -- the hull the
    library sets at a reneighbouring holds that box -- and the domain's own nlocal + nghost), so the read bins on cells
    1.26 or 1.26^2 times wider and the 5-cell stencil reaches further than it has to.  The histogram holds a full first
    shell: at 300 K every Mo has its 6 S inside 2.8 A (tests/test_gpu_adf_mdp.py), 12 ordered pairs per Mo; the alloy runs
    at 10 K: at 100 K its nearest-neighbour distances (2.86 A) spread by 0.07 A and 2 % of them lie beyond 3.0 A (the
    reference's figure, on the device's positions); the spread goes with the root of the temperature, 0.02 A at 10 K, and
    3.0 A is then six of them away: 12 per atom, less 1 % at the most."""
    s, v0 = _system(style, 300.0 if style == "rebomos" else 10.0)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        cutoff = SMALL_CUTOFF[style]
        d.rdf(NBIN, cutoff, PAIRS)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        nall = _nall(ctx)
        cells, grown = nets.measure_bin_grid(nets.measure_domain_lens(s.box, cutghost), cutoff, nall)
        first = nets.measure_bin_grid(nets.measure_domain_lens(s.box, cutghost), cutoff, 10 ** 9)[0]
        assert grown >= 1 and first[0] * first[1] * first[2] > 4 * nall + 4096, (first, nall)
        hist, ic, jc, du = d.rdf_read()
        ref = rdfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, cutoff, NBIN, RANGES)
        with capsys.disabled():
            print(f"{style}: cutoff {cutoff} A, nall {nall}, {first} cells of cutoff / 2 against the cap {4 * nall + 4096}, grown {grown} times to "
                  f"{cells}; {int(hist[0].sum())} pairs, {ref['n_edge']} edge pairs")
        rdfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"]) and np.array_equal(jc, ref["jcount"]) and np.array_equal(du, ref["dup"])
        n1 = int((s.type == 1).sum())
        if style == "rebomos":
            assert hist[2].sum() == hist[3].sum() == 6 * n1 and hist[0].sum() >= 12 * n1
        else:
            assert 0.99 * 12 * s.n <= hist[0].sum() <= 12 * s.n
    finally:
        ctx.close()


def test_one_workgroup_walks_every_chunk(monkeypatch, capsys):
    """MDP_MEASURE_GRID = 1 and 3 on the (3, 3, 2) MoS2 replica, 5 184 atoms and more than 64 x 256 owned and ghost atoms (the
    premise, from the domain): one workgroup takes more than 64 chunks, so it flushes its LDS counters inside its loop and
    goes on counting, and three take a third each.  Either read is in the reference's bracket and equals the read without
    the knob, integer for integer."""
    s = S.replicate(S.rebomos_bulk_cell(), (3, 3, 2))
    v0 = S.gaussian_velocities(s, 300.0, seed=3)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        monkeypatch.delenv("MDP_MEASURE_GRID", raising=False)
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        cutoff = 6.0
        d.rdf(NBIN, cutoff, PAIRS)
        d.compute(0, 0)
        for _ in range(5):
            d.step(0, 0, rebuild="auto")
        nall = _nall(ctx)
        assert nall > 16384 and s.n == 5184, nall
        plain = d.rdf_read()
        ref = rdfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, cutoff, NBIN, RANGES)
        rdfref.check_bracket(plain[0], ref)
        assert plain[0].sum() > 1e5
        for knob in ("1", "3", "0", ""):          # ("0" and "": the launch as it is)
            monkeypatch.setenv("MDP_MEASURE_GRID", knob)
            got = d.rdf_read()
            with capsys.disabled():
                print(f"MDP_MEASURE_GRID={knob!r}: nall {nall}, {-(-nall // 256)} chunks, differs from the plain read in "
                      f"{int((got[0] != plain[0]).sum())} counters")
            rdfref.check_bracket(got[0], ref)
            assert all(np.array_equal(a, b) for a, b in zip(got, plain)), knob
    finally:
        ctx.close()


def test_a_non_periodic_dimension(capsys):
    """the alloy with free z at 2 500 K: atoms leave the box in z (asserted, as tests/test_gpu_profile_mdp.py asserts it) and
    sit in clamped edge cells of the measurement grid; nobody has images in z, and the reference has none either"""
    s, v0 = _system("aeam", 2500.0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, nonperiodic=(0, 0, 1))
        cutoff = cutghost - skin
        d.rdf(NBIN, cutoff, PAIRS)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        hist, ic, jc, du = d.rdf_read()
        x = _x_by_tag(d, s.n)
        lamz = s.box.x2lamda(x)[:, 2]
        below, above = int((lamz < 0.0).sum()), int((lamz >= 1.0).sum())
        assert below > 5 and above >= 0 and below + above < s.n // 4, (below, above)
        ref = rdfref.counts(x, s.type, s.box.h, (1, 1, 0), cutoff, NBIN, RANGES)
        wrapped = rdfref.counts(x, s.type, s.box.h, PER, cutoff, NBIN, RANGES)
        with capsys.disabled():
            print(f"{below} atoms below and {above} above the box in z; {int(hist[0].sum())} pairs, {int(wrapped['hist'][0].sum())} with images in z")
        rdfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"]) and np.array_equal(jc, ref["jcount"]) and np.array_equal(du, ref["dup"])
        # the two faces have lost their partners: an atom at depth z < R under a face loses the cap (2 R^3 - 3 R^2 z + z^3) / (4 R^3)
        # of its sphere, 0.1875 R / L of all pairs per face in the mean: 10 % for R = 6.5 and L = 24.27 A
        assert 0.8 < hist[0].sum() / wrapped["hist"][0].sum() < 0.95 and hist[0].sum() > 4e4
    finally:
        ctx.close()


# ---- the drift case of tests/test_gpu_msd_mdp.py: the (2, 2, 2) MoS2 replica, 2 304 atoms, 300 K plus (60, -45, 30) A/ps,
# 40 steps, reneighbourings forced every 5
MIG_DRIFT, MIG_STEPS, MIG_RENB, MIG_READS = (60.0, -45.0, 30.0), 40, 5, (20, 40)


def _mig_system():
    s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 2))
    v0 = S.gaussian_velocities(s, 300.0, seed=8) + np.array(MIG_DRIFT)
    vcap = float(np.sqrt((v0 ** 2).sum(axis=1)).max()) + 5.0 * np.sqrt(S.BOLTZ * 300.0 / (float(s.mass[1:3].min()) * S.MVV2E))
    assert int(0.3 * 2.0 / (vcap * 0.001)) >= MIG_RENB       # no atom moves 0.3 skin between two builds
    return s, v0


def _mig_member(s):
    """every Mo, and the S atoms above the mid-plane of the box: by tag, as the whole system sees it"""
    return (s.type == 1) | (s.x[:, 2] > s.box.lo[2] + 0.5 * s.box.prd[2])


def _mig_run(s, v0, world, member):
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            cutoff = cutghost - skin
            d.rdf(NBIN, cutoff, PAIRS)
            d.compute(0, 0)
            out = {}
            for step in range(1, MIG_STEPS + 1):
                d.step(0, 0, rebuild=step % MIG_RENB == 0)
                if step in MIG_READS:
                    tags = d.tags_local
                    out[step] = dict(tags=tags.copy(), x=ctx.md_download(d.nlocal, want=("x",))["x"], rdf=d.rdf_read())
            d.rdf(NBIN, cutoff, PAIRS, member_by_tag=member)      # replaces the measurement of all atoms
            out["group"] = d.rdf_read()
            return dict(out=out, cutoff=cutoff)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    merged = dict(cutoff=res[0]["cutoff"])
    for key in MIG_READS + ("group",):
        got = [r["out"][key] if key == "group" else r["out"][key]["rdf"] for r in res]
        assert all(np.array_equal(a, b) for g in got for a, b in zip(g, got[0]))      # every rank reads the same sums
        merged[key] = dict(rdf=got[0])
        if key != "group":
            x, owner, seen = np.zeros((s.n, 3)), np.zeros(s.n, dtype=int), np.zeros(s.n, dtype=int)
            for k, r in enumerate(res):
                o = r["out"][key]
                x[o["tags"] - 1], owner[o["tags"] - 1] = o["x"], k
                seen[o["tags"] - 1] += 1
            assert np.all(seen == 1)
            merged[key].update(x=x, owner=owner)
    return merged


def test_bricks(capsys):
    """1, 2 and 8 bricks of the thread transport, reads at steps 20 and 40 and one more with a member table (every Mo and the
    S atoms above the mid-plane).  The rank-summed histograms of 2 and 8 bricks lie in the bracket of the reference on the
    one-brick positions and equal the one-brick histogram wherever no edge pair is adjacent; atoms change owner between
    the reads."""
    s, v0 = _mig_system()
    member = _mig_member(s)
    assert 0.6 * s.n < member.sum() < 0.75 * s.n
    one = _mig_run(s, v0, 1, member)
    cutoff = one["cutoff"]
    refs = {step: rdfref.counts(one[step]["x"], s.type, s.box.h, PER, cutoff, NBIN, RANGES) for step in MIG_READS}
    refs["group"] = rdfref.counts(one[MIG_READS[-1]]["x"], s.type, s.box.h, PER, cutoff, NBIN, RANGES, member)
    for world in (1, 2, 8):
        run = one if world == 1 else _mig_run(s, v0, world, member)
        for key in MIG_READS + ("group",):
            hist, ic, jc, du = run[key]["rdf"]
            ref = refs[key]
            with capsys.disabled():
                print(f"{world} bricks, {key}: {int(hist[0].sum())} pairs in * *, {ref['n_edge']} edge pairs, "
                      f"differs from one brick in {int((hist != one[key]['rdf'][0]).sum())} counters")
            rdfref.check_bracket(hist, ref)
            assert np.array_equal(ic, ref["icount"]) and np.array_equal(jc, ref["jcount"]) and np.array_equal(du, ref["dup"])
            free = ref["edge_adjacent"] == 0
            assert np.array_equal(hist[free], one[key]["rdf"][0][free])
            assert hist[0].sum() > 1e5
        if world > 1:
            moved = int((run[MIG_READS[0]]["owner"] != run[MIG_READS[-1]]["owner"]).sum())
            assert len(set(run[MIG_READS[-1]]["owner"])) == world and moved >= 3, moved
    assert refs["group"]["icount"][0] == member.sum() and refs["group"]["hist"][0].sum() < refs[MIG_READS[-1]]["hist"][0].sum()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_a_read_leaves_the_run_alone(style, capsys):
    """30 steps at 2 500 K with a histogram set up and read every 3 steps, and 30 steps without: x and v by tag are bit for
    bit the same, and so are the numbers of list builds (reneighbourings, the statistics of the last neighbour build with
    the style-list builds in them, prunings of the tile rows) -- a read bins on buffers of its own and touches nothing
    the steps or the list builders read.  Bit for bit asks for a run that repeats itself bit for bit: the three-body
    forces of the alloy's Si atoms are summed with float atomics (tests/test_gpu_group_mdp.py), so the aeam case runs
    the fcc metal without Si, whose kernels have none.  The run without reads is done twice and the test prints how far
    two plain runs are apart, next to the figure it asserts."""
    s, v0 = _system(style, 2500.0, seed=11, frac_si=0.0)
    states = []
    for measure in (True, False, False):
        ctx, st, skin, cutghost, map_ = _context(style)
        try:
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
            if measure:
                d.rdf(NBIN, cutghost - skin, PAIRS)
            d.compute(0, 0)
            total = 0
            for step in range(1, 31):
                d.step(0, 0, rebuild="auto")
                if measure and step % 3 == 0:
                    total += int(d.rdf_read()[0][0].sum())
            assert total > 1e5 or not measure
            tags = d.tags_local
            got = ctx.md_download(d.nlocal, want=("x", "v"))
            builds = (d.builds, tuple(ctx.md_neighbor_stats()), ctx.md_prune_stats()["prunings"])
            states.append((_by_tag(s.n, tags, got["x"]), _by_tag(s.n, tags, got["v"]), builds))
        finally:
            ctx.close()
    with capsys.disabled():
        print(f"{style}: with reads against without |dx| {np.abs(states[0][0] - states[1][0]).max():.2e} A, |dv| "
              f"{np.abs(states[0][1] - states[1][1]).max():.2e}; two runs without reads |dx| {np.abs(states[1][0] - states[2][0]).max():.2e} A; "
              f"builds {states[0][2]} / {states[1][2]}")
    # the premise: the run repeats itself bit for bit, so a difference above could only come from the reads
    assert np.array_equal(states[1][0], states[2][0]) and np.array_equal(states[1][1], states[2][1]) and states[1][2] == states[2][2]
    assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])
    assert states[0][2] == states[1][2] and states[0][2][0] >= 1, (states[0][2], states[1][2])


def test_refusals():
    s = S.rebomos_bulk_cell()
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        limit = cutghost - skin
        assert ctx.rdf_info() == dict(on=False, nbin=0, npair=0, serial=0)
        with pytest.raises(capi.MdpError, match="mdp_rdf_setup not called") as e:
            ctx.rdf_counts()
        assert e.value.code == ESTATE
        bad = [
            (dict(nbin=0), "nbin must be >= 1"),
            (dict(pairs=[]), "npair must be 1 .. 32"),
            (dict(pairs=[(1, 1, 1, 1)] * 33), "npair must be 1 .. 32"),
            (dict(pairs=[(0, 1, 1, 1)]), "type 0 outside 1 .. 2"),
            (dict(pairs=[(1, 1, 1, 3)]), "type 3 outside 1 .. 2"),
            (dict(pairs=[(2, 1, 1, 1)]), "lo > hi"),
            (dict(cutoff=0.0), "cutoff must be > 0"),
            (dict(cutoff=-1.0), "cutoff must be > 0"),
            (dict(cutoff=limit + 0.01), "exceeds the ghost shell"),
            (dict(nbin=4097, pairs=[(1, 1, 1, 1)] * 2), "the histogram in LDS holds 8192"),
        ]
        for kw, text in bad:
            args = dict(nbin=NBIN, cutoff=limit, pairs=[(1, 2, 1, 2)])
            args.update(kw)
            with pytest.raises(capi.MdpError, match=text) as e:
                ctx.rdf_setup(args["nbin"], args["cutoff"], args["pairs"])
            assert e.value.code == EINVAL, (kw, e.value.code)
        assert not ctx.rdf_info()["on"]
        ctx.rdf_setup(4096, limit, [(1, 1, 1, 1)] * 2)                       # the cap itself is accepted
        first = ctx.rdf_info()
        ctx.rdf_setup(NBIN, limit, [(1, 2, 1, 2)])                            # a second setup replaces the first
        second = ctx.rdf_info()
        assert first["on"] and second["on"] and second["serial"] > first["serial"] and (second["nbin"], second["npair"]) == (NBIN, 1)
        assert ctx.rdf_counts()[0].shape == (1, NBIN)
        # a member table shorter than a tag of the brick: reported at the read
        ctx.rdf_setup(NBIN, limit, [(1, 2, 1, 2)], member_by_tag=np.ones(s.n - 1, dtype=bool))
        with pytest.raises(capi.MdpError, match=rf"tag outside 1 .. {s.n - 1}") as e:
            ctx.rdf_counts()
        assert e.value.code == EINVAL
        ctx.rdf_setup(NBIN, limit, [(1, 2, 1, 2)], member_by_tag=np.ones(s.n, dtype=bool))
        assert ctx.rdf_counts()[1].tolist() == [s.n]
        ctx.rdf_off()
        assert not ctx.rdf_info()["on"]
        with pytest.raises(capi.MdpError, match="mdp_rdf_setup not called") as e:       # a read after mdp_rdf_off
            ctx.rdf_counts()
        assert e.value.code == ESTATE and d.nlocal == s.n
    finally:
        ctx.close()
    # without mdp_dd_setup, and without mdp_md_setup
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        with pytest.raises(capi.MdpError, match="mdp_md_setup not called") as e:
            ctx.rdf_setup(NBIN, 5.0, [(1, 2, 1, 2)])
        assert e.value.code == ESTATE
        cfg = capi.MdConfig()
        cfg.style, cfg.nlocal, cfg.nghost, cfg.ntypes = st, s.n, 0, 2
        cfg.skin, cfg.dt, cfg.ftm2v, cfg.mvv2e, cfg.nghost_self = skin, 0.001, S.FTM2V, S.MVV2E, 0
        for k in range(3):
            cfg.bbox_lo[k], cfg.bbox_hi[k] = -30.0, 60.0
        e3, e1 = np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
        ctx.md_setup(cfg, s.x, np.zeros_like(s.x), s.type, s.tag, s.mass, map_, e1, e3, e1, e1)
        with pytest.raises(capi.MdpError, match="mdp_dd_setup not called") as e:
            ctx.rdf_setup(NBIN, 5.0, [(1, 2, 1, 2)])
        assert e.value.code == ESTATE
        with pytest.raises(capi.MdpError, match="mdp_dd_setup not called"):
            ctx.rdf_counts()
    finally:
        ctx.close()
