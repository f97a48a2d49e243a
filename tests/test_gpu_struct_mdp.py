"""GPU: per-atom coordination numbers and the centro-symmetry parameter on the device (mdp_coord_*, mdp_centro_*, csrc/coord.hip,
csrc/centro.hip; DeviceDomain.coord / coord_read / centro / centro_read) against tests/structref.py, the NumPy brute force, on
positions downloaded by tag from the SAME device state.  The device compiles with -ffp-contract=fast and forms ghost
positions as x + shift, so the last bit of rsq may differ from NumPy's and nothing else.
  coord   count_sure <= device <= count_sure + edge for every atom and column (structref), which is equality wherever the
          reference has no pair within 1e-9 relative of the cutoff; every test caps the reference's edge pairs at 2.
  centro  |device - reference| <= 64 eps N Rc Lmax (structref.centro_bound, derived there: 2.8e-11 A^2 on the alloy at Rc = 6.5)
          for every atom whose choice of the N nearest is not ambiguous; every test caps the ambiguous atoms at 2.
All states are thermal: lattice distances at 0 K tie (tests/test_structref.py).  Every case reads twice (bit-identical), runs
over a group (atoms outside it are exactly 0) and checks that the returned tags are the owned tags.

Worst |device - reference| of centro seen on an MI355X (printed by every test): see DESIGN.md section 5."""
import numpy as np
import pytest

from conftest import POT_AEAM
from lammps_plugins_amd.host import capi, resident, system as S
import structref
from test_gpu_rdf_mdp import _by_tag, _context, _mig_system, _system, _x_by_tag, MIG_RENB, MIG_STEPS

pytestmark = pytest.mark.gpu

PER = (1, 1, 1)
EINVAL, ESTATE = -1, -6                     # MDP_EINVAL, MDP_ESTATE of include/mdpair_hip.h
GBIT = 2
COLS = [(1, 2), (1, 1), (2, 2)]             # *, 1, 2
COORD_RC = {"rebomos": 2.8, "aeam": 3.5}    # above the first shells (2.41 A Mo-S, 2.86 A fcc) and below the second
CENTRO = {"rebomos": (6, 4.0), "aeam": (12, None)}    # N and cutoff (None: the ghost shell's limit)


def _member(n):
    """four atoms of five, by tag: row t - 1"""
    return np.arange(1, n + 1) % 5 != 0


def _set_group(d, member):
    mask = np.ones(len(member) + 1, dtype=np.int32)
    mask[1:][member] |= GBIT
    d.set_group(mask, 1)                    # (bit 1: every atom is integrated)


def _lmax(s):
    return float(np.linalg.norm(s.box.h, axis=0).max())


def _read_both(d, n):
    """coord and centro twice each, by tag; asserts what every case asserts of a read"""
    out = []
    owned = np.sort(d.tags_local)
    for read in (d.coord_read, d.centro_read):
        tags, val = read()
        tags2, val2 = read()
        assert np.array_equal(tags, tags2) and np.array_equal(val, val2) and val.dtype == np.float64
        assert np.array_equal(np.sort(tags), owned) and np.array_equal(tags, d.tags_local)
        out.append(_by_tag(n, tags, val))
    return out


def _check_coord(dev, ref, member, max_edge=2):
    assert ref["n_edge"] <= max_edge, ref["n_edge"]
    lo, hi = ref["count_sure"], ref["count_sure"] + ref["edge"]
    assert np.array_equal(dev, np.rint(dev)) and np.all(dev[~member] == 0.0)
    bad = np.argwhere((dev < lo) | (dev > hi))
    assert len(bad) == 0, [(int(i), int(m), float(dev[i, m]), int(lo[i, m]), int(hi[i, m])) for i, m in bad[:8]]


def _check_centro(dev, ref, member, bound, max_ambiguous=2):
    """returns the worst |device - reference| over the atoms compared"""
    ok = ~ref["ambiguous"]
    assert int(ref["ambiguous"].sum()) <= max_ambiguous, int(ref["ambiguous"].sum())
    assert np.all(dev[~member] == 0.0)
    err = np.abs(dev - ref["value"])[ok]
    worst = int(np.argmax(err))
    assert err.max() <= bound, (float(err.max()), bound, float(dev[ok][worst]), float(ref["value"][ok][worst]))
    return float(err.max())


@pytest.mark.parametrize("temp", [300.0, 2500.0])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_brick(style, temp, capsys):
    """25 steps with no forced rebuild, so the reads happen with ghosts as old as the run leaves them.  coord at 2.8 / 3.5 A with the
    columns *, 1, 2; centro at N = 6 with cutoff 4.0 (MoS2) and N = 12 at the default cutoff, the ghost shell's limit (the alloy).
    Not vacuous, at 300 K: every Mo of the group has exactly 6 in column `2` and every S exactly 3 in column `1`; the alloy's
    all-types count is 12 for more than 99 % of the group."""
    s, v0 = _system(style, temp)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        nnn, rc = CENTRO[style]
        d.coord(COORD_RC[style], COLS, group_bit=GBIT)
        d.centro(nnn, rc, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        co, ce = _read_both(d, s.n)
        x = _x_by_tag(d, s.n)
        rc = cutghost - skin if rc is None else rc
        cref = structref.coord(x, s.type, s.box.h, PER, COORD_RC[style], COLS, member)
        zref = structref.centro(x, s.box.h, PER, nnn, rc, member)
        _check_coord(co, cref, member)
        bound = structref.centro_bound(nnn, rc, _lmax(s))
        worst = _check_centro(ce, zref, member, bound)
        few = ctx.centro_info()["few"]
        with capsys.disabled():
            print(f"{style} {temp:.0f} K: {d.builds} list builds; coord {cref['n_edge']} edge pairs; centro N {nnn} Rc {rc:.4f}: "
                  f"{int(zref['ambiguous'].sum())} ambiguous, worst |device - reference| {worst:.2e} A^2 (bound {bound:.2e}), "
                  f"largest value {ce.max():.3f} A^2, {few} centres short of N")
        assert few == int(((zref["inside"] < nnn) & member).sum()) and ce[member].max() > 1e-3
        assert np.array_equal(co[:, 0], co[:, 1] + co[:, 2])
        if temp == 300.0 and style == "rebomos":
            mo, su = member & (s.type == 1), member & (s.type == 2)
            assert np.all(co[mo, 2] == 6) and np.all(co[su, 1] == 3) and mo.sum() > 100 and su.sum() > 200
        if temp == 300.0 and style == "aeam":
            assert (co[member, 0] == 12).mean() > 0.99 and co[member, 2].max() >= 1
    finally:
        ctx.close()


def test_the_vacancy_stands_out(capsys):
    """the alloy with one atom removed (863 atoms, tags 1 .. 863) after 25 steps from 100 K: the vacancy's 12 neighbours hold the 12
    largest centro values, and their coordination number inside 3.5 A is 11"""
    full, _ = _system("aeam", 100.0)
    gone = 431
    dd = full.x - full.x[gone]
    dd -= np.rint(dd / full.box.prd) * full.box.prd
    near = np.nonzero(np.abs((dd * dd).sum(axis=1) - 0.5 * 4.045 ** 2) < 1e-6)[0]
    keep = np.arange(full.n) != gone
    near = near - (near > gone)
    s = S.System(full.box, np.ascontiguousarray(full.x[keep]), full.type[keep].copy(), np.arange(1, full.n, dtype=np.int32), full.mass)
    v0 = S.gaussian_velocities(s, 100.0, seed=3)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.coord(3.5)
        d.centro("fcc")
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        everyone = np.ones(s.n, dtype=bool)
        co, ce = _read_both(d, s.n)
        x = _x_by_tag(d, s.n)
        zref = structref.centro(x, s.box.h, PER, 12, cutghost - skin)
        worst = _check_centro(ce, zref, everyone, structref.centro_bound(12, cutghost - skin, _lmax(s)))
        _check_coord(co, structref.coord(x, s.type, s.box.h, PER, 3.5, [(1, 2)]), everyone)
        rest = np.setdiff1d(np.arange(s.n), near)
        with capsys.disabled():
            print(f"vacancy's neighbours {ce[near].min():.2f} .. {ce[near].max():.2f} A^2, the rest at most {ce[rest].max():.2f} A^2; "
                  f"worst |device - reference| {worst:.2e} A^2")
        assert len(near) == 12 and set(np.argsort(ce)[-12:]) == set(near)
        assert np.all(co[near, 0] == 11) and (co[rest, 0] == 12).all()
    finally:
        ctx.close()


def test_exact_ties_and_the_open_cutoff():
    """The one 0 K state: 8 x 8 x 8 cells of fcc with a = 4.0 A.  The box edge is 32 A, a power of two, so the coordinates, the way
    through reduced coordinates and back, the image shifts and the squared distances are all exact in binary, and nothing here
    is decided by rounding.  The six second neighbours lie at rsq = 16 = Rc^2 for Rc = 4.0: rsq < Rc^2 leaves them out --
    coord reads 12, not 18, and N = 18 finds 12 inside and reads 0 with every atom counted short; a hair more cutoff takes them
    in.  The 12 first neighbours all have rsq = 8 and their 66 pair values are 0 (six times), 8, 16, 24 and 32 in ties: the ranks
    break every tie on the index, each slot of the short lists is written exactly once, and the parameter is exactly 0."""
    s = S.fcc_cell(4.0, 8, frac_type2=0.05, seed=92)
    s.mass[1:3] = capi.AeamFile(POT_AEAM).mass[:2]
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        d.coord(4.0)
        tags, val = d.coord_read()
        assert np.all(val == 12.0) and val.shape == (s.n, 1)
        d.coord(4.0 + 1e-9)
        assert np.all(d.coord_read()[1] == 18.0)
        d.centro("fcc", 3.5)
        assert np.all(d.centro_read()[1] == 0.0) and ctx.centro_info()["few"] == 0
        d.centro("fcc")                                        # 78 inside 6.5 A, the 12 nearest in a 12-fold tie apart from the rest
        assert np.all(d.centro_read()[1] == 0.0) and ctx.centro_info()["few"] == 0
        d.centro(18, 4.0)
        assert np.all(d.centro_read()[1] == 0.0) and ctx.centro_info()["few"] == s.n
        d.centro(18, 4.0 + 1e-9)                               # 12 + 6, nine opposite pairs
        assert np.all(d.centro_read()[1] == 0.0) and ctx.centro_info()["few"] == 0
        d.centro(14, 4.0 + 1e-9)                               # 12 + 2 of the 6 tied second neighbours: the choice falls on the place; the seventh
                                                               # smallest pair value is 0 (the two are opposite) or 8 (a 120-degree pair)
        first = d.centro_read()[1]
        assert np.array_equal(first, d.centro_read()[1]) and set(np.unique(first)) <= {0.0, 8.0}
    finally:
        ctx.close()


# ---- the slots test_one_brick leaves empty
EIGHT = (5, 3)                # the alloy relabelled to 5 metal and 3 angular types: 36 inclusive type ranges, 32 of them taken
RANGES32 = [(lo, hi) for lo in range(1, 9) for hi in range(lo, 9)][:32]
_EIGHT = {}


def _eight_types():
    """the 864-atom alloy with 30 % Si relabelled to 8 types (five types have 15 inclusive ranges only: 32 columns of them could not
    all differ), as test_gpu_rdf_mdp._five_types relabels it to five"""
    import os
    import tempfile
    import aeam_five
    if not _EIGHT:
        nmet, nang = EIGHT
        path = os.path.join(tempfile.mkdtemp(), "eight.aeam")
        aeam_five.write_relabelled_file(path, POT_AEAM, [0] * nmet + [1] * nang, ["M%d" % i for i in range(nmet)] + ["X%d" % i for i in range(nang)])
        af = capi.AeamFile(path)
        s2 = S.fcc_cell(4.045, 6, frac_type2=0.3, seed=92)
        r = np.random.default_rng(5)
        ty = np.where(s2.type == 1, r.integers(1, nmet + 1, s2.n), r.integers(nmet + 1, nmet + nang + 1, s2.n)).astype(np.int32)
        _EIGHT.update(af=af, tabs=af.build(), s=S.System(s2.box, s2.x.copy(), ty, s2.tag.copy(), np.array([0.0] + list(af.mass))))
    s = _EIGHT["s"]
    return s, S.gaussian_velocities(s, 300.0, seed=3), _EIGHT["af"], _EIGHT["tabs"]


def test_32_columns(capsys):
    """32 pairwise different type ranges, all a mask word holds: column 32 (mask bit 31) is not empty and no two columns are equal"""
    s, v0, af, tabs = _eight_types()
    assert len(set(RANGES32)) == 32 and len(np.unique(s.type)) == 8
    member = _member(s.n)
    ctx = capi.Context(0)
    ctx.aeam_set_tables(tabs)
    skin, cutghost = 1.0, float(af.cut_table(tabs).max()) + 1.0
    try:
        d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, s, cutghost, skin, None, v0=v0)
        _set_group(d, member)
        d.coord(3.5, RANGES32, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        tags, val = d.coord_read()
        assert val.shape == (s.n, 32) and ctx.coord_info()["ncol"] == 32
        co = _by_tag(s.n, tags, val)
        ref = structref.coord(_x_by_tag(d, s.n), s.type, s.box.h, PER, 3.5, RANGES32, member)
        _check_coord(co, ref, member)
        with capsys.disabled():
            print(f"column 32 (types {RANGES32[31]}): {int(co[:, 31].sum())} partners in all, {ref['n_edge']} edge pairs")
        assert co[:, 31].sum() > 100 and len({co[:, m].tobytes() for m in range(32)}) == 32
    finally:
        ctx.close()


@pytest.mark.parametrize("nnn", [2, 64])
def test_the_smallest_and_the_largest_n(nnn, capsys):
    """N = 2 (one pair value) and N = 64 (2 016 of them, 32 per lane, all the pair values a wave keeps) on the alloy at its limit"""
    s, v0 = _system("aeam", 300.0)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        rc = cutghost - skin
        d.centro(nnn, None, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        tags, val = d.centro_read()
        assert np.array_equal(val, d.centro_read()[1])
        ce = _by_tag(s.n, tags, val)
        ref = structref.centro(_x_by_tag(d, s.n), s.box.h, PER, nnn, rc, member)
        bound = structref.centro_bound(nnn, rc, _lmax(s))
        worst = _check_centro(ce, ref, member, bound)
        with capsys.disabled():
            print(f"N = {nnn}: worst |device - reference| {worst:.2e} A^2 (bound {bound:.2e}), values up to {ce.max():.3f} A^2")
        assert ref["inside"].min() >= nnn and ce[member].min() > 0.0 and ctx.centro_info() == dict(on=True, nnn=nnn, few=0, serial=ctx.centro_info()["serial"])
    finally:
        ctx.close()


def test_small_groups_a_short_cutoff_and_one_workgroup(monkeypatch, capsys):
    """on one state of the alloy at 300 K: a group of two atoms; a group that is nobody (all zeros, no fault); N = 12 inside 2.9 A,
    where the atoms with fewer than 12 partners get 0 and are counted in mdp_centro_info; MDP_MEASURE_GRID = 1, one workgroup
    that walks every chunk, reads what the plain launch reads"""
    s, v0 = _system("aeam", 300.0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        monkeypatch.delenv("MDP_MEASURE_GRID", raising=False)
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        rc = cutghost - skin
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        x = _x_by_tag(d, s.n)
        bound = structref.centro_bound(12, rc, _lmax(s))
        for member in (np.isin(np.arange(1, s.n + 1), (7, 500)), np.zeros(s.n, dtype=bool)):
            _set_group(d, member)
            d.coord(3.5, COLS, group_bit=GBIT)
            d.centro("fcc", None, group_bit=GBIT)
            co, ce = _read_both(d, s.n)
            _check_coord(co, structref.coord(x, s.type, s.box.h, PER, 3.5, COLS, member), member)
            _check_centro(ce, structref.centro(x, s.box.h, PER, 12, rc, member), member, bound)
            assert int((co[:, 0] > 0).sum()) == int(member.sum()) == int((ce > 0).sum())
        member = _member(s.n)
        _set_group(d, member)
        d.centro(12, 2.9, group_bit=GBIT)
        co, ce = _read_both(d, s.n)
        ref = structref.centro(x, s.box.h, PER, 12, 2.9, member)
        short = member & (ref["inside"] < 12)
        _check_centro(ce, ref, member, structref.centro_bound(12, 2.9, _lmax(s)))
        with capsys.disabled():
            print(f"N = 12 inside 2.9 A: {int(short.sum())} of {int(member.sum())} centres have fewer than 12 partners")
        assert 10 < short.sum() < member.sum() and np.all(ce[short] == 0.0) and ctx.centro_info()["few"] == short.sum()
        assert np.all(ce[member & ~short & ~ref["ambiguous"]] > 0.0)
        # one workgroup for all chunks (more than one: the premise)
        d.coord(3.5, COLS, group_bit=GBIT)
        d.centro("fcc", None, group_bit=GBIT)
        plain = _read_both(d, s.n)
        info = ctx.dd_info()
        assert info["nlocal"] + info["nself"] + info["nrecv"] > 4 * 256
        for knob in ("1", "3"):
            monkeypatch.setenv("MDP_MEASURE_GRID", knob)
            got = _read_both(d, s.n)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), knob
        _check_coord(plain[0], structref.coord(x, s.type, s.box.h, PER, 3.5, COLS, member), member)
        _check_centro(plain[1], structref.centro(x, s.box.h, PER, 12, rc, member), member, bound)
    finally:
        ctx.close()


def test_a_non_periodic_dimension(capsys):
    """the alloy with free z at 2 500 K: atoms leave the box in z and sit in clamped edge cells of the measurement grid; nobody has
    images in z, the reference has none either, and the atoms of the two faces have lost partners"""
    s, v0 = _system("aeam", 2500.0)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, nonperiodic=(0, 0, 1))
        _set_group(d, member)
        rc = cutghost - skin
        d.coord(3.5, COLS, group_bit=GBIT)
        d.centro("fcc", None, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        co, ce = _read_both(d, s.n)
        x = _x_by_tag(d, s.n)
        lamz = s.box.x2lamda(x)[:, 2]
        assert int((lamz < 0.0).sum()) > 5
        cref = structref.coord(x, s.type, s.box.h, (1, 1, 0), 3.5, COLS, member)
        _check_coord(co, cref, member)
        worst = _check_centro(ce, structref.centro(x, s.box.h, (1, 1, 0), 12, rc, member), member, structref.centro_bound(12, rc, _lmax(s)))
        wrapped = structref.coord(x, s.type, s.box.h, PER, 3.5, COLS, member)["count_sure"]
        with capsys.disabled():
            print(f"free z: {int(co[:, 0].sum())} partners, {int(wrapped[:, 0].sum())} with images in z; worst centro error {worst:.2e} A^2")
        assert 0.9 < co[:, 0].sum() / wrapped[:, 0].sum() < 0.99
    finally:
        ctx.close()


@pytest.mark.parametrize("style,rc,nnn", [("aeam", None, 12), ("aeam", 3.5, 12), ("rebomos", 2.8, 6)])
def test_three_reads_of_one_walk(style, rc, nnn):
    """coord, adf and centro at one radius on one thermal state, no group and no member table: the three kernels walk the same
    candidates (csrc/measure_walk.h) and test the same rsq against the same rc^2, so with c_i = coord's count of atom i over all
    types, adf's `* * *` histogram over both shells [0, rc) holds sum_i c_i (c_i - 1) ordered angles of nlocal centres, and centro
    counts exactly the atoms with c_i < N short, which read 0 -- all exact, in integers.  Only a pair within one rounding of rc
    could tell the kernels apart, which a thermal state rules out (the module's docstring).  The alloy at the ghost shell's
    limit (None) has 78 partners, two trips of the walk per centre, at 3.5 A one; MoS2 at 2.8 A has empty runs across the van
    der Waals gap."""
    s, v0 = _system(style, 300.0)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        rc = cutghost - skin if rc is None else rc
        ntypes = int(s.type.max())
        d.coord(rc, [(1, ntypes)])
        d.adf(45, [((1, ntypes), (1, ntypes), (1, ntypes), 0.0, rc, 0.0, rc)])
        d.centro(nnn, rc)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        tags, val = d.coord_read()
        c = [int(v) for v in val[:, 0]]
        assert np.array_equal(val[:, 0], c) and len(c) == d.nlocal == s.n and max(c) >= nnn
        hist, icount = d.adf_read()
        assert int(hist.sum()) == sum(k * (k - 1) for k in c) and icount.tolist() == [s.n]
        ztags, z = d.centro_read()
        short = val[:, 0] < nnn
        assert np.array_equal(ztags, tags) and ctx.centro_info()["few"] == int(short.sum())
        assert np.all(z[short] == 0.0) and np.all(z[~short] >= 0.0)
    finally:
        ctx.close()


# ---- bricks: the drift case of tests/test_gpu_rdf_mdp.py, 2 304 MoS2 atoms, reneighbourings forced every 5 steps
def _mig_run(s, v0, world, member):
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            _set_group(d, member)
            d.coord(2.8, COLS, group_bit=GBIT)
            d.centro(6, 4.0, group_bit=GBIT)
            d.compute(0, 0)
            first = d.tags_local.copy()
            for step in range(1, MIG_STEPS + 1):
                d.step(0, 0, rebuild=step % MIG_RENB == 0)
            tags = d.tags_local.copy()
            ct, cv = d.coord_read()
            zt, zv = d.centro_read()
            assert np.array_equal(ct, tags) and np.array_equal(zt, tags)
            assert np.array_equal(cv, d.coord_read()[1]) and np.array_equal(zv, d.centro_read()[1])
            return dict(first=first, tags=tags, x=ctx.md_download(d.nlocal, want=("x",))["x"], coord=cv, centro=zv)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    seen = np.zeros(s.n, dtype=int)
    for r in res:
        seen[r["tags"] - 1] += 1
    assert np.all(seen == 1)
    cat = lambda k: np.concatenate([r[k] for r in res])
    tags = cat("tags")
    moved = sum(len(np.setdiff1d(r["tags"], r["first"])) for r in res)
    return dict(x=_by_tag(s.n, tags, cat("x")), coord=_by_tag(s.n, tags, cat("coord")), centro=_by_tag(s.n, tags, cat("centro")), moved=moved)


def test_bricks(capsys):
    """1, 2 and 8 bricks of the thread transport after 40 steps of drift with migration: by tag, coord is in the bracket of the
    reference on the run's own positions (equal where the reference has no edge pair) and centro within the bound"""
    s, v0 = _mig_system()
    member = _member(s.n)
    bound = structref.centro_bound(6, 4.0, _lmax(s))
    one = None
    for world in (1, 2, 8):
        run = _mig_run(s, v0, world, member)
        one = one or run
        cref = structref.coord(run["x"], s.type, s.box.h, PER, 2.8, COLS, member)
        zref = structref.centro(run["x"], s.box.h, PER, 6, 4.0, member)
        _check_coord(run["coord"], cref, member)
        worst = _check_centro(run["centro"], zref, member, bound)
        with capsys.disabled():
            print(f"{world} bricks: {run['moved']} atoms changed owner; coord {cref['n_edge']} edge pairs, differs from one brick in "
                  f"{int((run['coord'] != one['coord']).sum())} entries; centro worst |device - reference| {worst:.2e} A^2 (bound {bound:.2e}), "
                  f"against one brick {np.abs(run['centro'] - one['centro']).max():.2e}")
        mo = member & (s.type == 1)
        assert np.all(run["coord"][mo, 2] == 6) and run["centro"][member].max() > 1e-3
        assert world == 1 or run["moved"] >= 3


def test_refusals():
    """each returns MDP_EINVAL or MDP_ESTATE and a message, and leaves the context usable"""
    s, v0 = _system("rebomos", 300.0)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        limit = cutghost - skin
        assert ctx.coord_info() == dict(on=False, ncol=0, groupbit=0, serial=0)
        assert ctx.centro_info() == dict(on=False, nnn=0, few=0, serial=0)
        for read, text in ((ctx.coord_read, "mdp_coord_setup not called"), (ctx.centro_read, "mdp_centro_setup not called")):
            with pytest.raises(capi.MdpError, match=text) as e:
                read(d.nlocal)
            assert e.value.code == ESTATE
        bad_coord = [
            (dict(cutoff=limit + 0.01), "exceeds the ghost shell"),
            (dict(cutoff=0.0), "cutoff must be > 0"),
            (dict(ranges=[(1, 1)] * 33), "ncol must be 1 .. 32"),
            (dict(ranges=[]), "ncol must be 1 .. 32"),
            (dict(ranges=[(0, 1)]), "type 0 outside 1 .. 2"),
            (dict(ranges=[(1, 3)]), "type 3 outside 1 .. 2"),
            (dict(ranges=[(2, 1)]), "lo > hi"),
        ]
        for kw, text in bad_coord:
            args = dict(cutoff=2.8, ranges=[(1, 2)])
            args.update(kw)
            with pytest.raises(capi.MdpError, match=text) as e:
                ctx.coord_setup(args["cutoff"], args["ranges"])
            assert e.value.code == EINVAL, kw
        for nnn, rc, text in ((7, 4.0, "must be even"), (0, 4.0, "must be 2 .. 64"), (66, 4.0, "must be 2 .. 64"), (200, 4.0, "must be 2 .. 64"),
                              (6, limit + 0.01, "exceeds the ghost shell")):
            with pytest.raises(capi.MdpError, match=text) as e:
                ctx.centro_setup(nnn, rc)
            assert e.value.code == EINVAL, nnn
        assert not ctx.coord_info()["on"] and not ctx.centro_info()["on"]
        with pytest.raises(capi.MdpError, match="no mask covers the current atoms") as e:     # a group bit and no mask
            ctx.coord_setup(2.8, [(1, 2)], GBIT)
        assert e.value.code == ESTATE
        # MoS2 at the default cutoff (the shell's limit, 10.5 A): every centre has more than 128 atoms inside
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        ctx.centro_setup(6)
        with pytest.raises(capi.MdpError, match=r"more than 128 atoms inside the cutoff .*use a smaller cutoff") as e:
            ctx.centro_read(d.nlocal)
        assert e.value.code == EINVAL
        # ... and the context is as usable as before: the next read with cutoff 4.0 is right
        ctx.centro_setup(6, 4.0)
        tags, val = ctx.centro_read(d.nlocal)
        x = _x_by_tag(d, s.n)
        everyone = np.ones(s.n, dtype=bool)
        _check_centro(_by_tag(s.n, tags, val), structref.centro(x, s.box.h, PER, 6, 4.0), everyone, structref.centro_bound(6, 4.0, _lmax(s)))
        ctx.coord_setup(2.8, [(2, 2)])
        tags, val = ctx.coord_read(d.nlocal)
        assert np.all(_by_tag(s.n, tags, val)[s.type == 1, 0] == 6)
        first = ctx.coord_info()
        ctx.coord_setup(2.8, [(1, 1), (2, 2)])                       # a second setup replaces the first
        assert ctx.coord_info()["serial"] > first["serial"] and ctx.coord_info()["ncol"] == 2
        ctx.coord_off()
        ctx.centro_off()
        assert not ctx.coord_info()["on"] and not ctx.centro_info()["on"]
        with pytest.raises(capi.MdpError, match="mdp_centro_setup not called"):
            ctx.centro_read(d.nlocal)
    finally:
        ctx.close()
    # without mdp_md_setup
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        with pytest.raises(capi.MdpError, match="mdp_md_setup not called") as e:
            ctx.coord_setup(2.8, [(1, 2)])
        assert e.value.code == ESTATE
        with pytest.raises(capi.MdpError, match="mdp_md_setup not called"):
            ctx.centro_setup(6, 4.0)
    finally:
        ctx.close()
