"""GPU: the per-atom common neighbour analysis on the device (mdp_cna_*, csrc/cna.hip; DeviceDomain.cna / cna_read) against
tests/cnaref.py, the NumPy brute force, on positions downloaded by tag from the SAME device state.  Every result is a small
integer, so the tests demand equality.  The device compiles with -ffp-contract=fast and forms ghost positions as x + shift, so
the last bit of an rsq may differ from NumPy's and nothing else: an atom one of whose distances lies within 1e-9 relative of
the cutoff is AMBIGUOUS (cnaref) and not compared; the constructed cells may have none, the thermal runs at most 2.
Every case reads twice (bit-identical), runs over a four-of-five group (atoms outside it are exactly 0), checks that the
returned tags are the owned tags in order and that mdp_cna_counts is the histogram of the values handed out."""
import numpy as np
import pytest

from lammps_plugins_amd.host import capi, resident, system as S
import cnaref
from test_gpu_rdf_mdp import _by_tag, _context, _mig_system, _system, _x_by_tag, MIG_RENB, MIG_STEPS
from test_gpu_struct_mdp import _member, _set_group, EINVAL, ESTATE, GBIT, PER

pytestmark = pytest.mark.gpu


def _read(d, n):
    """two reads of one state, by tag; asserts what every case asserts of a read itself"""
    tags, val = d.cna_read()
    tags2, val2 = d.cna_read()
    assert np.array_equal(tags, tags2) and np.array_equal(val, val2) and val.dtype == np.float64
    assert np.array_equal(tags, d.tags_local) and np.array_equal(np.sort(tags), np.arange(1, n + 1))
    assert np.array_equal(val, np.rint(val)) and val.min() >= 0.0 and val.max() <= 5.0
    return _by_tag(n, tags, val).astype(np.int64)


def _check(d, dev, ref, member, max_ambiguous):
    """the device against the reference and against its own census; returns the device's histogram over the group"""
    nambig = int(ref["ambiguous"].sum())
    assert nambig <= max_ambiguous, nambig
    assert np.all(dev[~member] == 0) and np.all(dev[member] >= 1)
    ok = ~ref["ambiguous"]
    bad = np.nonzero(ok & (dev != ref["pattern"]))[0]
    assert len(bad) == 0, [(int(i) + 1, int(dev[i]), int(ref["pattern"][i]), int(ref["neighbours"][i])) for i in bad[:8]]
    hist = np.bincount(dev[member], minlength=6)
    counts = d.ctx.cna_counts()
    assert counts.tolist() == hist.tolist() and counts[0] == 0 and counts.sum() == member.sum()
    return hist


def _static_system(x, h):
    """one type of the alloy's at the positions x, wrapped into the orthorhombic box h"""
    box = S.Box(np.zeros(3), np.asarray(h).diagonal().copy(), np.zeros(3))
    n = len(x)
    mass = np.array([0.0] + list(capi.AeamFile(_pot()).mass[:2]))
    return S.System(box, S.wrap(box, x), np.ones(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), mass)


def _pot():
    from conftest import POT_AEAM
    return POT_AEAM


STATIC = {
    "stack": (lambda: cnaref.stack_cell()[:2], cnaref.RC_FCC),
    "bcc": (lambda: cnaref.bcc_cell(), cnaref.RC_BCC),
    "icosahedron": (lambda: cnaref.icosahedron_cell(), cnaref.RC_ICO),
}


@pytest.mark.parametrize("cell", sorted(STATIC))
def test_static_cells(cell, capsys):
    """the constructed cells of tests/test_cnaref.py, read after the setup compute with no steps: the close-packed stack holds
    both fcc and hcp, the bcc cell bcc, and the 13-atom cluster exactly one icosahedral atom.  No atom may be ambiguous."""
    make, rc = STATIC[cell]
    x, h = make()
    s = _static_system(x, h)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        _set_group(d, member)
        d.cna(rc, group_bit=GBIT)
        d.compute(0, 0)
        dev = _read(d, s.n)
        ref = cnaref.cna(_x_by_tag(d, s.n), s.box.h, PER, rc, member)
        hist = _check(d, dev, ref, member, 0)
        with capsys.disabled():
            print(f"{cell}: {s.n} atoms, Rc {rc:.4f}: patterns 0 .. 5 of the group {hist.tolist()}")
        present = set(ref["pattern"][member].tolist())
        if cell == "stack":
            assert {cnaref.FCC, cnaref.HCP} <= present and hist.tolist() == [0, 384, 384, 0, 0, 0]
        elif cell == "bcc":
            assert present == {cnaref.BCC}
        else:
            assert member[0] and int((ref["pattern"] == cnaref.ICO).sum()) == 1 and dev[0] == cnaref.ICO
        assert ctx.cna_info()["over"] == 0
    finally:
        ctx.close()


def test_exact_ties_and_the_open_cutoff():
    """The one state decided by no rounding: 8 x 8 x 8 cells of fcc with a = 4.0 A in a box of 32 A, where coordinates, image shifts
    and squared distances are exact in binary.  With Rc = 4.0 the six second neighbours lie at rsq = 16 = Rc^2, and so do the
    first neighbours across a square of the lattice from each other: rsq < Rc^2 leaves both out, 12 neighbours with (4,2,1,1)
    each, fcc.  A hair more cutoff takes them in: 18 neighbours, `other`, all counted over the list.  (Every atom is ambiguous
    for the reference, which is why it is not asked.)"""
    s = S.fcc_cell(4.0, 8)
    s.mass[1:3] = capi.AeamFile(_pot()).mass[:2]
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        d.cna(4.0)
        assert np.all(_read(d, s.n) == cnaref.FCC) and ctx.cna_counts().tolist() == [0, s.n, 0, 0, 0, 0] and ctx.cna_info()["over"] == 0
        d.cna(4.0 + 1e-9)
        assert np.all(_read(d, s.n) == cnaref.OTHER) and ctx.cna_counts().tolist() == [0, 0, 0, 0, 0, s.n] and ctx.cna_info()["over"] == s.n
    finally:
        ctx.close()


def test_thermal_alloy(capsys):
    """the 864-atom alloy with 5 % Si at 300 K after 25 steps: equality with the reference on the run's own positions, and fcc
    occurs (how much of the cell reads fcc after a real trajectory is printed, not asserted)"""
    s, v0 = _system("aeam", 300.0)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        d.cna(cnaref.RC_FCC, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        dev = _read(d, s.n)
        ref = cnaref.cna(_x_by_tag(d, s.n), s.box.h, PER, cnaref.RC_FCC, member)
        hist = _check(d, dev, ref, member, 2)
        with capsys.disabled():
            print(f"alloy 300 K, 25 steps: patterns 0 .. 5 of the group {hist.tolist()}, neighbours {np.bincount(ref['neighbours']).nonzero()[0].tolist()}, "
                  f"{int(ref['ambiguous'].sum())} ambiguous")
        assert hist[cnaref.FCC] > 0
    finally:
        ctx.close()


def test_hot_alloy_between_the_shells(capsys):
    """the alloy after 25 steps from 2 500 K with Rc = 3.9 A, where the second shell (4.045 A) has begun to cross the cutoff: with
    ballistic displacements of 0.5 to 1 times v0 t the reference finds 12 .. 17 neighbours, a tenth of the centres or more at
    15 or 16.  A centre with 15 or 16 neighbours fits the list and is not counted over it; one with 17 is.  The centres with 12
    or 14 take the whole path, and nearly all of them are `other`."""
    s, v0 = _system("aeam", 2500.0)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        d.cna(3.9, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        dev = _read(d, s.n)
        ref = cnaref.cna(_x_by_tag(d, s.n), s.box.h, PER, 3.9, member)
        hist = _check(d, dev, ref, member, 2)
        nn = ref["neighbours"][member]
        over, nambig = ctx.cna_info()["over"], int(ref["ambiguous"].sum())
        with capsys.disabled():
            print(f"alloy 2500 K, Rc 3.9: patterns {hist.tolist()}, neighbour counts {np.bincount(nn).tolist()}, {over} over 16, {nambig} ambiguous")
        assert abs(over - int((nn > 16).sum())) <= nambig
        assert ((nn == 15) | (nn == 16)).sum() > 0 and (nn == 12).sum() > 0 and (nn == 14).sum() > 0
        assert (ref["pattern"][member] == cnaref.OTHER).any()
    finally:
        ctx.close()


def test_the_vacancy(capsys):
    """the alloy with one atom removed (863 atoms, tags 1 .. 863) after 25 steps from 100 K: the vacancy's 12 neighbours have 11
    neighbours and read `other`"""
    full, _ = _system("aeam", 100.0)
    gone = 431
    dd = full.x - full.x[gone]
    dd -= np.rint(dd / full.box.prd) * full.box.prd
    near = np.nonzero(np.abs((dd * dd).sum(axis=1) - 0.5 * 4.045 ** 2) < 1e-6)[0]
    keep = np.arange(full.n) != gone
    near = near - (near > gone)
    s = S.System(full.box, np.ascontiguousarray(full.x[keep]), full.type[keep].copy(), np.arange(1, full.n, dtype=np.int32), full.mass)
    v0 = S.gaussian_velocities(s, 100.0, seed=3)
    member = np.ones(s.n, dtype=bool)
    member[4::5] = False
    member[near] = True                         # (four of five, and the twelve)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        d.cna(cnaref.RC_FCC, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        dev = _read(d, s.n)
        ref = cnaref.cna(_x_by_tag(d, s.n), s.box.h, PER, cnaref.RC_FCC, member)
        hist = _check(d, dev, ref, member, 2)
        with capsys.disabled():
            print(f"vacancy 100 K, 25 steps: patterns 0 .. 5 of the group {hist.tolist()}")
        assert len(near) == 12 and np.all(dev[near] == cnaref.OTHER) and np.all(ref["neighbours"][near] == 11)
        assert hist[cnaref.FCC] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("rc", [2.8, 3.5])
def test_off_the_close_packed_lattices(rc, capsys):
    """MoS2 at 300 K.  Inside 2.8 A a Mo has 6 neighbours and an S 3: every atom leaves at n not in {12, 14}.  Inside 3.5 A a Mo has
    6 S and 6 Mo, takes the whole path -- adjacency, signatures, ballots -- and must read `other` all the same."""
    s, v0 = _system("rebomos", 300.0)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        d.cna(rc, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        dev = _read(d, s.n)
        ref = cnaref.cna(_x_by_tag(d, s.n), s.box.h, PER, rc, member)
        hist = _check(d, dev, ref, member, 2)
        mo = member & (s.type == 1)
        with capsys.disabled():
            print(f"MoS2 Rc {rc}: patterns {hist.tolist()}, neighbours of Mo {sorted(set(ref['neighbours'][mo].tolist()))}, of S "
                  f"{sorted(set(ref['neighbours'][member & (s.type == 2)].tolist()))}")
        assert np.all(ref["neighbours"][mo] == (6 if rc == 2.8 else 12)) and mo.sum() > 100
        assert np.all(dev[member] == cnaref.OTHER) and ctx.cna_info()["over"] == 0
    finally:
        ctx.close()


def test_more_than_16_neighbours():
    """the alloy inside 4.2 A: 12 + 6 neighbours.  Every atom is `other`, never truncated into a pattern; info counts them all and
    the read succeeds"""
    s, v0 = _system("aeam", 300.0)
    member = _member(s.n)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        _set_group(d, member)
        d.cna(4.2, group_bit=GBIT)
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        dev = _read(d, s.n)
        ref = cnaref.cna(_x_by_tag(d, s.n), s.box.h, PER, 4.2, member)
        hist = _check(d, dev, ref, member, 2)
        assert np.all(ref["neighbours"] == 18) and np.all(dev[member] == cnaref.OTHER)
        info = ctx.cna_info()
        assert info["on"] and info["over"] == member.sum() == hist[cnaref.OTHER]
        d.cna(cnaref.RC_FCC, group_bit=GBIT)                  # ... and a second setup replaces the first, with a later serial
        assert ctx.cna_info()["serial"] > info["serial"] and ctx.cna_info()["over"] == 0 and ctx.cna_counts().sum() == 0
        assert _read(d, s.n)[member].min() >= 1 and ctx.cna_info()["over"] == 0
    finally:
        ctx.close()


# ---- bricks: the drift case of tests/test_gpu_rdf_mdp.py, 2 304 MoS2 atoms, reneighbourings forced every 5 steps
MIG_RC = 3.5                                    # a Mo takes the whole path


def _mig_run(s, v0, world, member):
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            _set_group(d, member)
            d.cna(MIG_RC, group_bit=GBIT)
            d.compute(0, 0)
            first = d.tags_local.copy()
            for step in range(1, MIG_STEPS + 1):
                d.step(0, 0, rebuild=step % MIG_RENB == 0)
            tags = d.tags_local.copy()
            t, v = d.cna_read()
            counts = ctx.cna_counts()
            assert np.array_equal(t, tags) and np.array_equal(v, d.cna_read()[1]) and np.array_equal(counts, ctx.cna_counts())
            mine = member[tags - 1]
            assert counts.tolist() == np.bincount(v[mine].astype(np.int64), minlength=6).tolist() and np.all(v[~mine] == 0.0)
            return dict(first=first, tags=tags, x=ctx.md_download(d.nlocal, want=("x",))["x"], cna=v, counts=counts)
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
    return dict(x=_by_tag(s.n, tags, cat("x")), cna=_by_tag(s.n, tags, cat("cna")).astype(np.int64), moved=moved,
                counts=sum(r["counts"] for r in res))


def test_bricks(capsys):
    """1, 2 and 8 bricks of the thread transport after 40 steps of drift with migration: by tag, every brick count reads what the
    reference reads on the run's own positions, the same as one brick, and the census summed over the bricks is the same"""
    s, v0 = _mig_system()
    member = _member(s.n)
    one = None
    for world in (1, 2, 8):
        run = _mig_run(s, v0, world, member)
        one = one or run
        ref = cnaref.cna(run["x"], s.box.h, PER, MIG_RC, member)
        assert int(ref["ambiguous"].sum()) <= 2
        ok = ~ref["ambiguous"]
        assert np.array_equal(run["cna"][ok], ref["pattern"][ok]) and np.all(run["cna"][~member] == 0)
        with capsys.disabled():
            print(f"{world} bricks: {run['moved']} atoms changed owner; census {run['counts'].tolist()}, {int(ref['ambiguous'].sum())} ambiguous, "
                  f"differs from one brick in {int((run['cna'] != one['cna']).sum())} atoms")
        assert np.array_equal(run["cna"][ok], one["cna"][ok]) and run["counts"].sum() == member.sum()
        assert ref["ambiguous"].any() or run["counts"].tolist() == one["counts"].tolist()
        assert np.all(ref["neighbours"][member & (s.type == 1)] == 12)
        assert world == 1 or run["moved"] >= 3


def test_refusals():
    """each returns MDP_EINVAL or MDP_ESTATE and a message, and leaves the context usable"""
    s, v0 = _system("aeam", 300.0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        limit = cutghost - skin
        assert ctx.cna_info() == dict(on=False, over=0, serial=0)
        for call in (lambda: ctx.cna_read(d.nlocal), ctx.cna_counts):                  # a read before the setup
            with pytest.raises(capi.MdpError, match="mdp_cna_setup not called") as e:
                call()
            assert e.value.code == ESTATE
        for rc, text in ((limit + 0.01, "exceeds the ghost shell"), (0.0, "cutoff must be > 0"), (-1.0, "cutoff must be > 0"),
                         (float("inf"), "cutoff must be > 0")):
            with pytest.raises(capi.MdpError, match=text) as e:
                ctx.cna_setup(rc)
            assert e.value.code == EINVAL, rc
        assert not ctx.cna_info()["on"]
        with pytest.raises(capi.MdpError, match="no mask covers the current atoms") as e:     # a group bit and no mask
            ctx.cna_setup(cnaref.RC_FCC, GBIT)
        assert e.value.code == ESTATE
        d.compute(0, 0)
        _set_group(d, _member(s.n))
        d.cna(cnaref.RC_FCC, group_bit=8)                       # a bit nobody carries: no centre, all zeros, an empty census
        tags, val = d.cna_read()
        assert np.array_equal(tags, d.tags_local) and np.all(val == 0.0) and ctx.cna_counts().tolist() == [0] * 6
        d.cna(cnaref.RC_FCC)                                    # ... and the context is as usable as before
        tags, val = d.cna_read()
        assert np.all(val == cnaref.FCC) and ctx.cna_counts().tolist() == [0, s.n, 0, 0, 0, 0]
        ctx.cna_off()
        assert ctx.cna_info() == dict(on=False, over=0, serial=0)
        with pytest.raises(capi.MdpError, match="mdp_cna_setup not called"):
            ctx.cna_read(d.nlocal)
    finally:
        ctx.close()
    ctx, st, skin, cutghost, map_ = _context("aeam")                # without mdp_md_setup
    try:
        with pytest.raises(capi.MdpError, match="mdp_md_setup not called") as e:
            ctx.cna_setup(cnaref.RC_FCC)
        assert e.value.code == ESTATE
    finally:
        ctx.close()
