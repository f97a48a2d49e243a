"""GPU: bond-angle histograms on the device (mdp_adf_*, csrc/adf.hip; DeviceDomain.adf / adf_read) against tests/adfref.py,
the NumPy brute force, on positions downloaded by tag from the SAME device state.  The device compiles with
-ffp-contract=fast, forms ghost positions as x + shift and the cosine as (d_ij . d_ik) (1 / r_ij) (1 / r_ik), so the last
bits of an ordinate may differ from NumPy's and nothing else: a device histogram is right when hist_sure <= device <=
hist_sure + edge_adjacent for every triple and bin (adfref), and every test requires of the reference at most 2 edge
angles and no neighbour at a shell radius (expected: below 1e-2 each for 1e5 - 5e6 angles and windows of 2e-9).  All
states are thermal: lattice angles at 0 K are the business of the plugin test, which puts them mid-bin.  The systems are
those of tests/test_gpu_rdf_mdp.py."""
import os
import re

import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS  # noqa: F401  (the potentials _context reads)
from lammps_plugins_amd.host import capi, resident, system as S
from test_gpu_rdf_mdp import (MIG_READS, MIG_RENB, MIG_STEPS, PAIRS, SMALL_CUTOFF, TYPE_RANGES, _by_tag, _context, _five_context,
                              _five_types, _mig_member, _mig_system, _nall, _system, _x_by_tag)
import adfref
import nets

pytestmark = pytest.mark.gpu

PER = (1, 1, 1)
NBIN = 45
EINVAL, ESTATE = -1, -6                     # MDP_EINVAL, MDP_ESTATE of include/mdpair_hip.h
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mdpair_hip.h")
MAXNEIGH = int(re.search(r"#define MDP_ADF_MAXNEIGH (\d+)", open(HEADER).read()).group(1))
ALL = (1, 2)


def _triples(style):
    """(itype, jtype, ktype, rjin, rjout, rkin, rkout): r1 lies between the first and the second shell of either lattice
    (MoS2: Mo-S 2.41, then S-S 3.1 and Mo-Mo 3.16; fcc: 2.86, then 4.045), r2 behind the second.
      0  * * *          first shell            3  2 * *   the S / Si centres: 0 = 3 + 4 partition * * * by the centre's type
      1  1 2 2 / 1 1 1  S-Mo-S / Al-Al-Al      4  1 * *   the Mo / Al centres
      2  2 1 1          Mo-S-Mo / Al-Si-Al     5  * * *   inner radius > 0: the second shell alone
      6  1 * 1          j in the first shell, k in the second: every (j, k) once, no (k, j)
      7  * * *          0 .. 0.5: an empty selection, whose centres still count"""
    r1, r2 = (2.8, 3.6) if style == "rebomos" else (3.5, 4.5)
    return [(ALL, ALL, ALL, 0.0, r1, 0.0, r1), (1, 2, 2, 0.0, r1, 0.0, r1) if style == "rebomos" else (1, 1, 1, 0.0, r1, 0.0, r1),
            (2, 1, 1, 0.0, r1, 0.0, r1), (2, ALL, ALL, 0.0, r1, 0.0, r1), (1, ALL, ALL, 0.0, r1, 0.0, r1),
            (ALL, ALL, ALL, r1, r2, r1, r2), (1, ALL, 1, 0.0, r1, r1, r2), (ALL, ALL, ALL, 0.0, 0.5, 0.0, 0.5)]


def _rows(triples):
    """the triples as adfref and capi take them: (ilo, ihi, jlo, jhi, klo, khi, rjin, rjout, rkin, rkout)"""
    rng = lambda t: (t, t) if np.ndim(t) == 0 else tuple(t)
    return [rng(t[0]) + rng(t[1]) + rng(t[2]) + tuple(t[3:]) for t in triples]


@pytest.mark.parametrize("temp", [300.0, 2500.0])
@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_brick(style, temp, capsys):
    """25 steps with no forced rebuild, so the read happens with ghosts as old as the run leaves them; 45 bins in degrees and
    the eight triples of _triples, then the same state once more in radians (MoS2) or in the cosine (alloy).  The device
    histogram inside the reference's bracket, icount exact, two reads identical, * * * the sum of its partition.  Not
    vacuous, from the lattice: at 300 K no Mo-S bond (2.41 A) reaches 2.8 A and no Mo-Mo distance (3.16 A) falls to it, so
    a Mo has its 6 S (30 ordered pairs) and an S its 3 Mo (6), exactly (an S may, rarely, see another S of 3.1 - 3.2 A
    inside 2.8 A: S * * is bounded, not fixed), and an fcc atom its 12 neighbours (132) within 3.5 A to within 1 %; at
    2 500 K the first shell still holds more than half of that."""
    s, v0 = _system(style, temp)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        tr = _triples(style)
        d.adf(NBIN, tr)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        hist, ic = d.adf_read()
        again = d.adf_read()
        assert np.array_equal(hist, again[0]) and np.array_equal(ic, again[1])
        assert hist.dtype == np.int64 and hist.shape == (len(tr), NBIN)
        x = _x_by_tag(d, s.n)
        ref = adfref.counts(x, s.type, s.box.h, PER, NBIN, "degree", _rows(tr))
        with capsys.disabled():
            print(f"{style} {temp:.0f} K: {d.builds} list builds, {int(hist[0].sum())} angles in * * *, {int(hist.sum())} in all, "
                  f"{ref['n_edge']} edge angles, {ref['n_shell_edge']} shell-edge neighbours, at most {ref['max_neighbours']} neighbours, "
                  f"device - reference {int(np.abs(hist - ref['hist']).sum())} counts")
        adfref.check_bracket(hist, ref)
        n1, n2 = int((s.type == 1).sum()), int((s.type == 2).sum())
        assert np.array_equal(ic, ref["icount"]) and ic.tolist() == [s.n, n1, n2, n2, n1, s.n, n1, s.n] and n2 > 0
        assert np.array_equal(hist[0], hist[3] + hist[4]) and hist[7].sum() == 0 and hist[5].sum() > 0 and hist[6].sum() > 0
        per1, per2 = (30, 6) if style == "rebomos" else (132, 132)
        if temp == 300.0 and style == "rebomos":
            assert hist[1].sum() == hist[4].sum() == per1 * n1 and hist[2].sum() == per2 * n2 <= hist[3].sum() < 1.1 * per2 * n2
        elif temp == 300.0:
            assert abs(hist[0].sum() / s.n - 132.0) < 1.32 and 0 < hist[2].sum() < hist[3].sum() < hist[1].sum() < hist[4].sum()
        else:
            assert hist[4].sum() > 0.5 * per1 * n1 and hist[3].sum() > 0.5 * per2 * n2
        arr = resident.adf_normalise(hist, ic, NBIN, "degree", "centre")
        assert np.allclose(arr, adfref.normalise(hist, ic, NBIN, "degree", "centre"), rtol=1e-13, atol=1e-13)
        assert np.allclose(resident.adf_normalise(hist, ic, NBIN), adfref.normalise(hist, ic, NBIN), rtol=1e-13, atol=1e-13)
        # the other two ordinates on the same state: radians share the bins of degrees, the cosine has its own
        other = "radian" if style == "rebomos" else "cosine"
        d.adf(NBIN, tr, ordinate=other)
        hist2, ic2 = d.adf_read()
        ref2 = adfref.counts(x, s.type, s.box.h, PER, NBIN, other, _rows(tr))
        adfref.check_bracket(hist2, ref2)
        assert np.array_equal(ic2, ic) and np.array_equal(hist2.sum(axis=1), hist.sum(axis=1))
        if other == "radian":
            free = (ref["edge_adjacent"] == 0) & (ref2["edge_adjacent"] == 0)
            assert np.array_equal(hist2[free], hist[free])
        else:
            assert not np.array_equal(hist2, hist)
    finally:
        ctx.close()


# ---- the slots test_one_brick leaves empty, as in tests/test_gpu_rdf_mdp.py
def _triples32():
    """32 triples over the 5 types of _five_types with pairwise different type ranges and shells: triple m takes every 97th
    of the 15^3 range triples, j-shell 0 .. 3.0 + 0.1 m (3.0 - 6.1 A), k-shell 0.05 m .. 6.4 - 0.1 m (6.4 - 3.3 A)"""
    all3 = [a + b + c for a in TYPE_RANGES for b in TYPE_RANGES for c in TYPE_RANGES][::97]
    return [all3[m] + (0.0, 3.0 + 0.1 * m, 0.05 * m, 6.4 - 0.1 * m) for m in range(32)]


def test_8192_counters_and_triple_32(capsys):
    """32 triples x 256 bins, all the LDS histogram holds, on the alloy relabelled to 5 types; triple 32 (mask bit 31) is not
    empty, and no two triples hold the same histogram"""
    s, v0, af, tabs = _five_types()
    rows = _triples32()
    assert len({r[:6] for r in rows}) == 32 and len({r[6:] for r in rows}) == 32
    ctx, st, skin, cutghost, map_ = _five_context()
    try:
        assert max(max(r[7], r[9]) for r in rows) < cutghost - skin
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.adf(256, [((r[0], r[1]), (r[2], r[3]), (r[4], r[5])) + r[6:] for r in rows])
        d.compute(0, 0)
        for _ in range(10):
            d.step(0, 0, rebuild="auto")
        hist, ic = d.adf_read()
        assert hist.shape == (32, 256) and ctx.adf_info()["nbin"] * ctx.adf_info()["ntriple"] == 8192
        ref = adfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, 256, "degree", rows)
        with capsys.disabled():
            print(f"{int(hist.sum())} angles, triple 32: {int(hist[31].sum())}, {ref['n_edge']} edge angles, at most {ref['max_neighbours']} neighbours")
        adfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"]) and ref["max_neighbours"] <= MAXNEIGH
        assert ref["hist_sure"][31].sum() > 1000 and all(ref["hist_sure"][m].sum() > 0 for m in range(32))
        assert len({ref["hist"][m].tobytes() for m in range(32)}) == 32
    finally:
        ctx.close()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_bin(style):
    """nbin = 1: the one counter of a triple is the number of its angles -- the reference's, and the sum of the 45 bins read
    on the same state (every angle lands in a bin: there is no cutoff on the ordinate)"""
    s, v0 = _system(style, 300.0)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        tr = _triples(style)
        d.compute(0, 0)
        for _ in range(5):
            d.step(0, 0, rebuild="auto")
        d.adf(1, tr, ordinate="cosine")
        one = d.adf_read()
        d.adf(NBIN, tr)
        many = d.adf_read()
        ref = adfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, 1, "cosine", _rows(tr))
        adfref.check_bracket(one[0], ref)
        assert ref["n_edge"] == 0                                     # (one bin has no interior edge)
        assert one[0].shape == (len(tr), 1) and np.array_equal(one[0], ref["hist"]) and one[0][0, 0] > 1e4
        assert np.array_equal(one[0][:, 0], many[0].sum(axis=1)) and np.array_equal(one[1], many[1])
    finally:
        ctx.close()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_a_small_outer_radius_widens_the_cells(style, capsys):
    """the largest outer radius just above the first shell: the premise and the systems of test_a_small_cutoff_widens_the_cells
    (tests/test_gpu_rdf_mdp.py).  A full first shell: 30 ordered pairs of S around every Mo, 6 of Mo around every S; 132 of
    the 12 nearest neighbours around an alloy atom, less 2.5 % at the most (1 % of the neighbours: 11.88 x 10.88 = 129.3)."""
    s, v0 = _system(style, 300.0 if style == "rebomos" else 10.0)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        r = SMALL_CUTOFF[style]
        tr = [(ALL, ALL, ALL, 0.0, r, 0.0, r), (1, 2, 2, 0.0, r, 0.0, r), (2, 1, 1, 0.0, r, 0.0, r), (1, ALL, ALL, 0.5 * r, r, 0.0, 0.9 * r)]
        d.adf(NBIN, tr)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        nall = _nall(ctx)
        lens = nets.measure_domain_lens(s.box, cutghost)
        cells, grown = nets.measure_bin_grid(lens, r, nall)
        first = nets.measure_bin_grid(lens, r, 10 ** 9)[0]
        assert grown >= 1 and first[0] * first[1] * first[2] > 4 * nall + 4096, (first, nall)
        hist, ic = d.adf_read()
        ref = adfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, NBIN, "degree", _rows(tr))
        with capsys.disabled():
            print(f"{style}: outer radius {r} A, nall {nall}, {first} cells against the cap {4 * nall + 4096}, grown {grown} times to {cells}; "
                  f"{int(hist[0].sum())} angles, {ref['n_edge']} edge angles")
        adfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"])
        n1, n2 = int((s.type == 1).sum()), int((s.type == 2).sum())
        if style == "rebomos":
            assert hist[1].sum() == 30 * n1 and hist[2].sum() == 6 * n2 and hist[0].sum() >= 30 * n1 + 6 * n2
        else:
            assert 0.975 * 132 * s.n <= hist[0].sum() <= 132 * s.n
    finally:
        ctx.close()


def test_one_workgroup_walks_every_chunk(monkeypatch, capsys):
    """MDP_MEASURE_GRID = 1 and 3 on the (3, 3, 2) MoS2 replica: the premise and the claim of the test of this name in
    tests/test_gpu_rdf_mdp.py, for the angle kernel's chunk loop and the flush inside it"""
    s = S.replicate(S.rebomos_bulk_cell(), (3, 3, 2))
    v0 = S.gaussian_velocities(s, 300.0, seed=3)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        monkeypatch.delenv("MDP_MEASURE_GRID", raising=False)
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        tr = _triples("rebomos")
        d.adf(NBIN, tr)
        d.compute(0, 0)
        for _ in range(5):
            d.step(0, 0, rebuild="auto")
        nall = _nall(ctx)
        assert nall > 16384 and s.n == 5184, nall
        plain = d.adf_read()
        ref = adfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, NBIN, "degree", _rows(tr))
        adfref.check_bracket(plain[0], ref)
        n1, n2 = int((s.type == 1).sum()), int((s.type == 2).sum())
        assert plain[0].sum(axis=1)[1:3].tolist() == [30 * n1, 6 * n2]
        for knob in ("1", "3", "0", ""):          # ("0" and "": the launch as it is)
            monkeypatch.setenv("MDP_MEASURE_GRID", knob)
            got = d.adf_read()
            with capsys.disabled():
                print(f"MDP_MEASURE_GRID={knob!r}: nall {nall}, {-(-nall // 256)} chunks, differs from the plain read in "
                      f"{int((got[0] != plain[0]).sum())} counters")
            adfref.check_bracket(got[0], ref)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), knob
    finally:
        ctx.close()


def test_a_non_periodic_dimension(capsys):
    """the alloy with free z at 2 500 K: atoms leave the box in z (asserted) and sit in clamped edge cells of the measurement
    grid; the reference has no images in z.  The first-shell angles are fewer than with images in z: the atoms of the two
    faces have lost neighbours."""
    s, v0 = _system("aeam", 2500.0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, nonperiodic=(0, 0, 1))
        tr = _triples("aeam")
        d.adf(NBIN, tr)
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        hist, ic = d.adf_read()
        x = _x_by_tag(d, s.n)
        lamz = s.box.x2lamda(x)[:, 2]
        below, above = int((lamz < 0.0).sum()), int((lamz >= 1.0).sum())
        assert below > 5 and above >= 0 and below + above < s.n // 4, (below, above)
        ref = adfref.counts(x, s.type, s.box.h, (1, 1, 0), NBIN, "degree", _rows(tr))
        wrapped = adfref.counts(x, s.type, s.box.h, PER, NBIN, "degree", _rows(tr))
        with capsys.disabled():
            print(f"{below} atoms below and {above} above the box in z; {int(hist[0].sum())} angles, {int(wrapped['hist'][0].sum())} with images in z")
        adfref.check_bracket(hist, ref)
        assert np.array_equal(ic, ref["icount"])
        assert 1e4 < hist[0].sum() < wrapped["hist"][0].sum()
    finally:
        ctx.close()


def test_more_neighbours_than_a_wave_has_lanes(capsys):
    """the alloy at 300 K with * * * over 0 .. cutghost - skin = 6.5 A: the 78 neighbours of five fcc shells, about 6 000 ordered
    pairs per atom and 5e6 in all -- the gather strides twice over its hits and the pair loop makes about 94 passes"""
    s, v0 = _system("aeam", 300.0)
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        r = cutghost - skin
        tr = [(ALL, ALL, ALL, 0.0, r, 0.0, r)]
        d.adf(NBIN, tr)
        d.compute(0, 0)
        for _ in range(5):
            d.step(0, 0, rebuild="auto")
        hist, ic = d.adf_read()
        ref = adfref.counts(_x_by_tag(d, s.n), s.type, s.box.h, PER, NBIN, "degree", _rows(tr))
        with capsys.disabled():
            print(f"{int(hist.sum())} angles, at most {ref['max_neighbours']} neighbours, {ref['n_edge']} edge angles, "
                  f"device - reference {int(np.abs(hist - ref['hist']).sum())} counts")
        assert 64 < ref["max_neighbours"] <= MAXNEIGH and hist.sum() > 4e6
        adfref.check_bracket(hist, ref)
        assert ic.tolist() == [s.n]
    finally:
        ctx.close()


def test_the_neighbour_cap(capsys):
    """MoS2 holds 0.057 atoms / A^3, so MAXNEIGH = 128 neighbours lie inside 8.1 A and every atom has more inside 9.05 A, well
    under cutghost - skin = 11.4 A: the read names the centres and the cap and hands nothing back; a setup with the first
    shell then reads right"""
    s, _ = _system("rebomos", 300.0)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        r = 9.05
        assert r < cutghost - skin and 0.057 * 4.0 / 3.0 * np.pi * r ** 3 > MAXNEIGH
        ni = adfref.neighbours(s.x, s.box.h, PER, r)[0]
        per_atom = np.bincount(ni, minlength=s.n)
        over = int((per_atom > MAXNEIGH).sum())
        with capsys.disabled():
            print(f"{per_atom.min()} .. {per_atom.max()} neighbours inside {r} A, {over} centres over the cap of {MAXNEIGH}")
        assert over == s.n and not np.any(np.abs(per_atom - MAXNEIGH) < 8)        # (nobody near the cap: a count, not a rounding)
        d.adf(NBIN, [(ALL, ALL, ALL, 0.0, r, 0.0, 2.8)])
        with pytest.raises(capi.MdpError, match=rf"{over} centres have more than {MAXNEIGH} neighbours.*use smaller outer radii") as e:
            d.adf_read()
        assert e.value.code == EINVAL
        d.adf(NBIN, [(1, 2, 2, 0.0, 2.8, 0.0, 2.8), (2, 1, 1, 0.0, 2.8, 0.0, 2.8)])
        hist, ic = d.adf_read()
        n1, n2 = int((s.type == 1).sum()), int((s.type == 2).sum())
        assert ic.tolist() == [n1, n2] and hist.sum(axis=1).tolist() == [30 * n1, 6 * n2]
    finally:
        ctx.close()


# ---- the drift case of tests/test_gpu_rdf_mdp.py: the (2, 2, 2) MoS2 replica, 300 K plus a drift, 40 steps, reneighbourings every 5
MIG_TRIPLES = [(ALL, ALL, ALL, 0.0, 2.8, 0.0, 2.8), (1, 2, 2, 0.0, 2.8, 0.0, 2.8), (2, 1, 1, 0.0, 2.8, 0.0, 2.8), (ALL, ALL, ALL, 0.0, 4.2, 2.8, 4.2)]


def _mig_run(s, v0, world, member):
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            d.adf(NBIN, MIG_TRIPLES)
            d.compute(0, 0)
            out = {}
            for step in range(1, MIG_STEPS + 1):
                d.step(0, 0, rebuild=step % MIG_RENB == 0)
                if step in MIG_READS:
                    out[step] = dict(tags=d.tags_local.copy(), x=ctx.md_download(d.nlocal, want=("x",))["x"], adf=d.adf_read())
            d.adf(NBIN, MIG_TRIPLES, member_by_tag=member)          # replaces the measurement of all atoms
            out["group"] = d.adf_read()
            return out
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    merged = {}
    for key in MIG_READS + ("group",):
        got = [r[key] if key == "group" else r[key]["adf"] for r in res]
        assert all(np.array_equal(a, b) for g in got for a, b in zip(g, got[0]))      # every rank reads the same sums
        merged[key] = dict(adf=got[0])
        if key != "group":
            x, owner, seen = np.zeros((s.n, 3)), np.zeros(s.n, dtype=int), np.zeros(s.n, dtype=int)
            for k, r in enumerate(res):
                x[r[key]["tags"] - 1], owner[r[key]["tags"] - 1] = r[key]["x"], k
                seen[r[key]["tags"] - 1] += 1
            assert np.all(seen == 1)
            merged[key].update(x=x, owner=owner)
    return merged


def test_bricks(capsys):
    """1, 2 and 8 bricks of the thread transport, reads at steps 20 and 40 and one more with a member table (every Mo and the
    S atoms above the mid-plane).  The rank-summed histograms lie in the bracket of the reference on the one-brick
    positions and equal the one-brick histogram wherever no edge angle is adjacent; atoms change owner between the reads."""
    s, v0 = _mig_system()
    member = _mig_member(s)
    one = _mig_run(s, v0, 1, member)
    rows = _rows(MIG_TRIPLES)
    refs = {step: adfref.counts(one[step]["x"], s.type, s.box.h, PER, NBIN, "degree", rows) for step in MIG_READS}
    refs["group"] = adfref.counts(one[MIG_READS[-1]]["x"], s.type, s.box.h, PER, NBIN, "degree", rows, member)
    n1, n2 = int((s.type == 1).sum()), int((s.type == 2).sum())
    for world in (1, 2, 8):
        run = one if world == 1 else _mig_run(s, v0, world, member)
        for key in MIG_READS + ("group",):
            hist, ic = run[key]["adf"]
            ref = refs[key]
            with capsys.disabled():
                print(f"{world} bricks, {key}: {int(hist.sum())} angles, {ref['n_edge']} edge angles, "
                      f"differs from one brick in {int((hist != one[key]['adf'][0]).sum())} counters")
            adfref.check_bracket(hist, ref)
            assert np.array_equal(ic, ref["icount"])
            free = ref["edge_adjacent"] == 0
            assert np.array_equal(hist[free], one[key]["adf"][0][free])
            if key != "group":
                assert hist.sum(axis=1)[1:3].tolist() == [30 * n1, 6 * n2] and hist[0].sum() >= 30 * n1 + 6 * n2 and hist[3].sum() > 1e5
        if world > 1:
            moved = int((run[MIG_READS[0]]["owner"] != run[MIG_READS[-1]]["owner"]).sum())
            assert len(set(run[MIG_READS[-1]]["owner"])) == world and moved >= 3, moved
    assert refs["group"]["icount"][0] == member.sum() and 0 < refs["group"]["hist"][0].sum() < refs[MIG_READS[-1]]["hist"][0].sum()


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_a_read_leaves_the_run_alone(style, capsys):
    """30 steps at 2 500 K with a histogram set up and read every 3 steps, and 30 steps without: x and v by tag are bit for
    bit the same, and so are the numbers of list builds, the statistics of the last neighbour build and the prunings of
    the tile rows.  The premise and the choice of the alloy without Si are those of tests/test_gpu_rdf_mdp.py: the run
    without reads is done twice, and must repeat itself bit for bit."""
    s, v0 = _system(style, 2500.0, seed=11, frac_si=0.0)
    tr = [_triples(style)[0], _triples(style)[5]]
    states = []
    for measure in (True, False, False):
        ctx, st, skin, cutghost, map_ = _context(style)
        try:
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
            if measure:
                d.adf(NBIN, tr)
            d.compute(0, 0)
            total = 0
            for step in range(1, 31):
                d.step(0, 0, rebuild="auto")
                if measure and step % 3 == 0:
                    total += int(d.adf_read()[0].sum())
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
    assert np.array_equal(states[1][0], states[2][0]) and np.array_equal(states[1][1], states[2][1]) and states[1][2] == states[2][2]
    assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])
    assert states[0][2] == states[1][2] and states[0][2][0] >= 1, (states[0][2], states[1][2])


def test_rdf_next_to_adf_on_one_context():
    """a context holds one measurement of each kind, each with a binning of its own at its own cell width: set up together
    and read in turns on one state, each reads what it reads alone on a context of its own"""
    s, v0 = _system("rebomos", 300.0)
    tr = _triples("rebomos")[:3]
    got = {}
    for which in ("both", "rdf", "adf"):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
            if which != "adf":
                d.rdf(50, cutghost - skin, PAIRS)
            if which != "rdf":
                d.adf(NBIN, tr)
            d.compute(0, 0)
            for _ in range(5):
                d.step(0, 0, rebuild="auto")
            reads = []
            for _ in range(2):                       # adf, rdf, adf, rdf: neither disturbs the other's buffers or setup
                if which != "rdf":
                    reads.append(("adf",) + tuple(d.adf_read()))
                if which != "adf":
                    reads.append(("rdf",) + tuple(d.rdf_read()))
            got[which] = reads
            info = (ctx.rdf_info()["on"], ctx.adf_info()["on"])
            assert info == (which != "adf", which != "rdf")
        finally:
            ctx.close()
    for kind in ("rdf", "adf"):
        alone = [r for r in got[kind] if r[0] == kind]
        both = [r for r in got["both"] if r[0] == kind]
        assert len(alone) == len(both) == 2
        for r in both + alone[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(r[1:], alone[0][1:]))
    assert got["adf"][0][1].sum() > 1e4 and got["rdf"][0][1].sum() > 1e5


def test_refusals():
    s = S.rebomos_bulk_cell()
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        limit = cutghost - skin
        assert ctx.adf_info() == dict(on=False, nbin=0, ntriple=0, serial=0)
        with pytest.raises(capi.MdpError, match="mdp_adf_setup not called") as e:
            ctx.adf_counts()
        assert e.value.code == ESTATE
        ok = (1, 2, 1, 2, 1, 2, 0.0, 2.8, 0.0, 2.8)
        tr = lambda **kw: [tuple(kw.get(k, v) for k, v in zip(("ilo", "ihi", "jlo", "jhi", "klo", "khi", "rjin", "rjout", "rkin", "rkout"), ok))]
        bad = [
            (dict(nbin=0), "nbin must be >= 1, not 0"),
            (dict(ordinate=3), "ordinate must be 0 .degree., 1 .radian. or 2 .cosine., not 3"),
            (dict(ordinate=-1), "ordinate must be .* not -1"),
            (dict(triples=[]), "ntriple must be 1 .. 32, not 0"),
            (dict(triples=[ok] * 33), "ntriple must be 1 .. 32, not 33"),
            (dict(triples=tr(ilo=0)), "triple 1: type 0 outside 1 .. 2"),
            (dict(triples=tr(khi=3)), "triple 1: type 3 outside 1 .. 2"),
            (dict(triples=[ok] + tr(jlo=2, jhi=1)), "triple 2: a type range with lo > hi"),
            (dict(triples=tr(rjin=-0.5)), "a radius must be >= 0, not -0.5"),
            (dict(triples=tr(rkin=2.8)), "the inner radius 2.8 is not below the outer radius 2.8"),
            (dict(triples=tr(rjin=3.0)), "the inner radius 3 is not below the outer radius 2.8"),
            (dict(triples=tr(rjout=limit + 0.01)), "exceeds the ghost shell"),
            (dict(triples=tr(rkout=limit + 0.01)), "exceeds the ghost shell"),
            (dict(nbin=4097, triples=[ok] * 2), "nbin x ntriple = 8194 counters, the histogram in LDS holds 8192"),
            (dict(member=np.zeros(0, dtype=bool)), "a member table with ntag = 0"),
        ]
        for kw, text in bad:
            args = dict(nbin=NBIN, ordinate="degree", triples=[ok], member=None)
            args.update(kw)
            with pytest.raises(capi.MdpError, match=text) as e:
                ctx.adf_setup(args["nbin"], args["ordinate"], args["triples"], args["member"])
            assert e.value.code == EINVAL, (kw, e.value.code)
        assert not ctx.adf_info()["on"]
        ctx.adf_setup(4096, "cosine", [ok] * 2)                              # the cap itself is accepted, and so is the limit
        first = ctx.adf_info()
        ctx.adf_setup(NBIN, "degree", tr(rjout=limit))                       # a second setup replaces the first
        second = ctx.adf_info()
        assert first["on"] and second["on"] and second["serial"] > first["serial"] and (second["nbin"], second["ntriple"]) == (NBIN, 1)
        ctx.adf_setup(NBIN, "degree", [ok])
        assert ctx.adf_counts()[0].shape == (1, NBIN)
        # a member table shorter than a tag of the brick: reported at the read
        ctx.adf_setup(NBIN, "degree", [ok], member_by_tag=np.ones(s.n - 1, dtype=bool))
        with pytest.raises(capi.MdpError, match=rf"tag outside 1 .. {s.n - 1}") as e:
            ctx.adf_counts()
        assert e.value.code == EINVAL
        ctx.adf_setup(NBIN, "degree", [ok], member_by_tag=np.ones(s.n, dtype=bool))
        assert ctx.adf_counts()[1].tolist() == [s.n]
        ctx.adf_off()
        assert not ctx.adf_info()["on"]
        with pytest.raises(capi.MdpError, match="mdp_adf_setup not called") as e:       # a read after mdp_adf_off
            ctx.adf_counts()
        assert e.value.code == ESTATE and d.nlocal == s.n
    finally:
        ctx.close()
    # without mdp_dd_setup, and without mdp_md_setup
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        with pytest.raises(capi.MdpError, match="mdp_md_setup not called") as e:
            ctx.adf_setup(NBIN, "degree", [ok])
        assert e.value.code == ESTATE
        cfg = capi.MdConfig()
        cfg.style, cfg.nlocal, cfg.nghost, cfg.ntypes = st, s.n, 0, 2
        cfg.skin, cfg.dt, cfg.ftm2v, cfg.mvv2e, cfg.nghost_self = skin, 0.001, S.FTM2V, S.MVV2E, 0
        for k in range(3):
            cfg.bbox_lo[k], cfg.bbox_hi[k] = -30.0, 60.0
        e3, e1 = np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
        ctx.md_setup(cfg, s.x, np.zeros_like(s.x), s.type, s.tag, s.mass, map_, e1, e3, e1, e1)
        with pytest.raises(capi.MdpError, match="mdp_adf_setup: mdp_dd_setup not called") as e:
            ctx.adf_setup(NBIN, "degree", [ok])
        assert e.value.code == ESTATE
        with pytest.raises(capi.MdpError, match="mdp_adf_counts: mdp_dd_setup not called"):
            ctx.adf_counts()
    finally:
        ctx.close()
