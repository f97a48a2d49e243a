"""GPU: the heat current on the device (mdp_heatflux_sums, mdp_md_download_vatom, csrc/heatflux.hip; DeviceDomain.heatflux)
against tests/heatfluxref.py on v, eatom, vatom and mass downloaded from the SAME device state, and against the CPU oracle's
per-atom tallies on the downloaded positions.

Bounds.  Kernel against its inputs: a 256-lane block sum plus a slot sum over at most 5 blocks (9 for the 2 304-atom case)
rounds below 3e-14 relative to the sum of the terms' magnitudes, so every sum must lie within 1e-12 * sum|term|.  Physics:
the project's per-atom tolerances against the oracle (eatom 1e-9 eV, vatom 1e-9 relative to max(1, max|vatom|)) carried
through the formula give sum_i |v_i|_1 * (1e-9 + 3e-9 * max(1, max|vatom|)) per component.  At 300 K with velocity seed 3
(the default of _system) the CPU oracle, run for the same 25 steps, gives |component| / bound of
  MoS2  (1 152 atoms): J 1.09e6, 3.6e5, 8.5e5; convective part 1.5e4, 3.3e4, 1.0e5
  alloy (864 atoms):   J 3.8e5, 6.8e5, 6.7e5;  convective part 1.3e5, 9.2e5, 1.6e5
so the comparison is far from vacuous (the tests assert a factor of 100).  Measured on one MI355X: device sums within
1.4e-17 (MoS2) and 1.9e-17 (alloy) of the exact ones relative to sum|term|; |device - oracle| at most 6.0e-8 and 1.2e-8 of
the physics bound; 2 and 4 bricks within 1.5e-16 and 2.1e-16 of one brick."""
import dataclasses
import math

import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
import heatfluxref
import mdref
from test_gpu_rdf_mdp import _by_tag, _context, _mig_system, _system, MIG_RENB, MIG_STEPS

pytestmark = pytest.mark.gpu

ENOTIMPL, ESTATE = -5, -6                   # MDP_ENOTIMPL, MDP_ESTATE of include/mdpair_hip.h
STYLES = ["rebomos", "aeam"]
_runs = {}


def _download(d):
    """v, eatom, vatom, mass, x and the tags of the device's current atoms, in device order"""
    got = d.ctx.md_download(d.nlocal, want=("x", "v", "eatom"))
    return dict(x=got["x"], v=got["v"], eatom=got["eatom"], vatom=d.ctx.md_download_vatom(d.nlocal), mass=d._mass_local(),
                tags=d.tags_local.copy())


def _run(style):
    """25 steps at 300 K (the device's own displacement check decides the rebuilds); the last is a tallying compute (eflag 3,
    vflag 5) with its final half deferred.  The first read is mdp_heatflux_sums itself, which has to complete that half.
    Run once per style and shared by the tests below, which only read it."""
    if style in _runs:
        return _runs[style]
    s, v0 = _system(style, 300.0)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.compute(0, 0)
        for k in range(25):
            last = k == 24
            d.step(3 if last else 0, 5 if last else 0, rebuild="auto", defer_final=last)
        out = ctx.heatflux_sums()           # (the library completes the deferred half: not DeviceDomain.flush)
        d._final_pending = False
        ke = d.thermo()["ke"]
        again = ctx.heatflux_sums()
        vec = d.heatflux()
        _runs[style] = dict(s=s, out=out, again=again, vec=vec, ke=ke, builds=d.builds, **_download(d))
    finally:
        ctx.close()
    return _runs[style]


@pytest.mark.parametrize("style", STYLES)
def test_kernel_against_its_own_inputs(style, capsys):
    r = _run(style)
    s, out = r["s"], r["out"]
    ref = heatfluxref.sums(r["mass"], r["v"], r["eatom"], r["vatom"], S.MVV2E)
    err = np.abs(out - ref["sums"]) / ref["mag"]
    with capsys.disabled():
        print(f"{style}: {r['builds']} list builds, J {np.array2string(r['vec'], precision=6)}, worst |device - exact| / sum|term| {err.max():.2e}")
    assert out[6] == s.n == ref["sums"][6]
    assert np.all(np.abs(out - ref["sums"]) <= 1e-12 * ref["mag"]), err
    assert np.array_equal(out, r["again"])
    assert np.array_equal(r["vec"], np.concatenate([out[0:3] + out[3:6], out[0:3]]))
    # the read completed the deferred half: out[7] = ke + sum eatom with the kinetic energy md_thermo reports afterwards.
    # (Relative to the magnitudes summed, as every sum here; a missing half-kick moves ke by about 1e-2 of itself.)
    assert r["ke"] > 0.0 and abs(out[7] - (r["ke"] + math.fsum(r["eatom"]))) <= 1e-12 * ref["mag"][7]
    ke_ref = S.kinetic_energy(r["mass"], r["v"])
    assert abs(r["ke"] - ke_ref) <= 1e-12 * ke_ref


@pytest.mark.parametrize("style", STYLES)
def test_physics_against_the_oracle(style, oracle, capsys):
    r = _run(style)
    s = r["s"]
    n, tags = s.n, r["tags"]
    x, v = _by_tag(n, tags, r["x"]), _by_tag(n, tags, r["v"])
    s2 = dataclasses.replace(s, x=S.wrap(s.box, x))
    if style == "rebomos":
        eng = mdref.RebomosCPU(oracle, oracle.rebomos_params(POT_REBOMOS), s2)
    else:
        eng = mdref.AeamCPU(oracle, oracle.aeam_pot(POT_AEAM), s2)
    o = eng.compute(s2.x)
    ea, va = o["eatom"][:n].copy(), o["vatom"][:n].copy()
    np.add.at(ea, eng.owner, o["eatom"][n:])         # the oracle's ghost shares onto their owners
    np.add.at(va, eng.owner, o["vatom"][n:])
    if style == "aeam":                              # angular centres whose rows cross the periodic faces: the fold is exercised
        assert np.abs(o["vatom"][n:]).max() > 1e-3
    scale = max(1.0, float(np.abs(va).max()))
    assert np.abs(_by_tag(n, tags, r["eatom"]) - ea).max() < 1e-9
    assert np.abs(_by_tag(n, tags, r["vatom"]) - va).max() < 1e-9 * scale
    ref = heatfluxref.sums(s.mass[s.type], v, ea, va, S.MVV2E)
    bound = float(np.abs(v).sum()) * (1e-9 + 3e-9 * scale)
    out = r["out"]
    diff = np.concatenate([np.abs(r["vec"] - ref["vector"]), np.abs(out[3:6] - ref["sums"][3:6])])
    with capsys.disabled():
        print(f"{style}: bound {bound:.3e}, worst |device - oracle| / bound {diff.max() / bound:.3e}, "
              f"least |component| / bound {np.abs(ref['vector']).min() / bound:.3e}")
    assert np.all(diff <= bound), diff / bound
    assert np.all(np.abs(ref["vector"]) > 100.0 * bound) and np.all(np.abs(ref["sums"][3:6]) > 100.0 * bound)


@pytest.mark.parametrize("style", STYLES)
def test_group(style):
    """the mask of `type 1, or above the mid-plane`: the count and the sums over the members only; a group bit without a mask
    is refused"""
    s, v0 = _system(style, 300.0)
    member = (s.type == 1) | (s.x[:, 2] > s.box.lo[2] + 0.5 * s.box.prd[2])
    assert 0.5 * s.n < member.sum() < s.n
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.compute(3, 5)
        with pytest.raises(capi.MdpError, match="no mask covers the current atoms") as e:
            ctx.heatflux_sums(group_bit=2)
        assert e.value.code == ESTATE
        mask = np.ones(s.n + 1, dtype=np.int32)
        mask[1:] |= 2 * member.astype(np.int32)
        d.set_group(mask, 1)
        for k in range(10):
            d.step(3 if k == 9 else 0, 5 if k == 9 else 0, rebuild="auto")
        out, everyone = ctx.heatflux_sums(group_bit=2), ctx.heatflux_sums()
        got = _download(d)
        mem = member[got["tags"] - 1]
        ref = heatfluxref.sums(got["mass"], got["v"], got["eatom"], got["vatom"], S.MVV2E, member=mem)
        assert out[6] == member.sum() == ref["sums"][6] and everyone[6] == s.n
        assert np.all(np.abs(out - ref["sums"]) <= 1e-12 * ref["mag"])
        assert np.abs(out[:6] - everyone[:6]).max() > 1e-3          # the other atoms carry their share
        assert np.array_equal(d.heatflux(group_bit=2), np.concatenate([out[0:3] + out[3:6], out[0:3]]))
        ctx.md_set_mask(None)                # the mask withdrawn under a read that needs it
        with pytest.raises(capi.MdpError, match="no mask covers the current atoms") as e:
            ctx.heatflux_sums(group_bit=2)
        assert e.value.code == ESTATE
    finally:
        ctx.close()


@pytest.mark.parametrize("style", STYLES)
def test_validity(style):
    """both reads are refused unless the last finished compute took eatom and vatom for the atoms as they are now"""
    s, v0 = _system(style, 300.0)
    ctx, st, skin, cutghost, map_ = _context(style)

    def refused(text):
        for read in (ctx.heatflux_sums, lambda: ctx.md_download_vatom(s.n)):
            with pytest.raises(capi.MdpError, match=text) as e:
                read()
            assert e.value.code == ESTATE

    def served():
        out = ctx.heatflux_sums()
        assert out[6] == s.n and np.abs(ctx.md_download_vatom(s.n)).max() > 0.0
        return out

    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        refused("tallies are stale")                     # set up, lists built, no compute yet
        d.compute(0, 0)
        refused("eflag 0, vflag 0")
        d.compute(1, 1)
        refused("eflag 1, vflag 1")
        d.compute(3, 1)
        refused("eflag 3, vflag 1")
        d.compute(1, 5)
        refused("eflag 1, vflag 5")
        d.compute(3, 5)
        first = served()
        d.step(0, 0)                                     # a plain step
        refused("eflag 0, vflag 0")
        d.step(3, 5)
        second = served()
        assert not np.array_equal(first[:6], second[:6])
        ctx.dd_reneighbor()                              # the atoms are re-ordered: the tallies belong to the old order
        refused("tallies are stale")
        d.compute(3, 5)
        third = served()
        # the same state in another atom order: the same sums up to the order of the additions
        ref = heatfluxref.sums(**{k: v for k, v in _download(d).items() if k in ("mass", "v", "eatom", "vatom")}, mvv2e=S.MVV2E)
        assert np.all(np.abs(third - second) <= 2e-12 * ref["mag"])
        ctx.md_initial_integrate()                       # the atoms move: the tallies describe the state they left
        refused("tallies are stale")
    finally:
        ctx.close()


def _bricks_run(s, v0, world):
    """MIG_STEPS steps of the drifting MoS2 replica with reneighbourings every MIG_RENB; the last step tallies"""
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            d.compute(0, 0)
            first = d.tags_local.copy()
            for step in range(1, MIG_STEPS + 1):
                last = step == MIG_STEPS
                d.step(3 if last else 0, 5 if last else 0, rebuild=step % MIG_RENB == 0)
            out = dict(sums=ctx.heatflux_sums(), vec=d.heatflux(), first=first, **_download(d))
            return out
        finally:
            ctx.close()

    return [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)


def test_bricks_rebomos(capsys):
    """1, 2 and 4 bricks of the thread transport with migration: the six values summed over the ranks equal the one-brick
    values within the bound of the sums, every rank reads the same total, the counts add to n, atoms changed owner"""
    s, v0 = _mig_system()
    one = _bricks_run(s, v0, 1)[0]
    ref = heatfluxref.sums(one["mass"], one["v"], one["eatom"], one["vatom"], S.MVV2E)
    assert one["sums"][6] == s.n and np.all(np.abs(one["sums"] - ref["sums"]) <= 1e-12 * ref["mag"])
    mag6 = np.concatenate([ref["mag"][0:3] + ref["mag"][3:6], ref["mag"][0:3]])
    for world in (2, 4):
        res = _bricks_run(s, v0, world)
        assert all(np.array_equal(r["vec"], res[0]["vec"]) for r in res)
        tot = np.sum([r["sums"] for r in res], axis=0)
        assert tot[6] == s.n and all(r["sums"][6] == len(r["tags"]) > 0 for r in res)
        assert len(np.unique(np.concatenate([r["tags"] for r in res]))) == s.n
        vec = res[0]["vec"]
        err = np.abs(vec - one["vec"]) / mag6
        moved = sum(len(np.setdiff1d(r["tags"], r["first"])) for r in res)
        with capsys.disabled():
            print(f"{world} bricks: worst |sum over ranks - one brick| / sum|term| {err.max():.2e}, {moved} atoms changed owner")
        assert np.all(np.abs(vec - one["vec"]) <= 1e-12 * mag6), err
        assert np.all(np.abs(tot - one["sums"]) <= 1e-12 * ref["mag"])
        assert moved >= 3


def test_bricks_aeam_are_refused_where_angular_centres_reach_remote_ghosts():
    """the alloy on 2 bricks: Si centres sit at the brick faces, the thirds of their triplets' virial land on remote ghosts,
    and both reads say so; the same calls on one rank succeed"""
    s, v0 = _system("aeam", 300.0)

    def rank_fn(r, make_tr, world=2):
        ctx, st, skin, cutghost, map_ = _context("aeam")
        try:
            tr = make_tr(ctx) if world > 1 else None
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            d.compute(3, 5)
            got = []
            for read in (ctx.heatflux_sums, lambda: ctx.md_download_vatom(d.nlocal)):
                try:
                    read()
                    got.append((0, ""))
                except capi.MdpError as e:
                    got.append((e.code, str(e)))
            return dict(got=got, remote=ctx.md_aeam_state()["ghost_forces"], nlocal=d.nlocal)
        finally:
            ctx.close()

    res = resident.run_ranks(2, rank_fn)
    assert sum(r["nlocal"] for r in res) == s.n
    for r in res:
        assert r["remote"]
        for code, text in r["got"]:
            assert code == ENOTIMPL and "remote ghosts" in text and "2 ranks" in text, (code, text)
    one = rank_fn(0, None, world=1)
    assert [c for c, _ in one["got"]] == [0, 0] and not one["remote"]


# ---- the slots the runs above leave empty: more than 256 slots for mdp_slot_total_kernel<8>, a group of nobody
@pytest.fixture(scope="module")
def big():
    """70 304 aluminium atoms (fcc 26^3, as the indenter's second-trip test), jittered by 0.05 A, at 300 K: 275 blocks.  Built
    once for this module."""
    s = S.fcc_cell(4.045, 26)
    s.mass[1:3] = capi.AeamFile(POT_AEAM).mass[:2]
    s = S.jitter(s, 0.05, seed=71)
    assert s.n == 70304 and -(-s.n // 256) == 275 and s.n % 256 == 160
    return s, S.gaussian_velocities(s, 300.0, seed=72)


def test_the_slot_sums_second_trip_against_fsum(big, capsys):
    """275 slots: mdp_slot_sum_256<8> takes a second trip.  One tallying compute, no step; the sums over all atoms and over
    the atoms with tag % 3 == 0 against heatfluxref.sums of the downloaded v, eatom, vatom and mass within 1e-12 of the
    terms' magnitudes (any order of adding n terms stays within n 2^-53 = 7.8e-12; a fixed tree does far better)"""
    s, v0 = big
    member = s.tag % 3 == 0
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        assert -(-d.nlocal // 256) > 256                                   # the premise: more slots than lanes
        mask = np.ones(s.n + 1, dtype=np.int32)
        mask[1:] |= 2 * member.astype(np.int32)
        d.set_group(mask, 0)
        d.compute(3, 5)
        got = _download(d)
        assert np.abs(got["vatom"]).max() > 1e-2 and np.abs(got["eatom"]).max() > 1.0
        worst = []
        for bit, mem in ((0, None), (2, member[got["tags"] - 1])):
            out, again = ctx.heatflux_sums(group_bit=bit), ctx.heatflux_sums(group_bit=bit)
            ref = heatfluxref.sums(got["mass"], got["v"], got["eatom"], got["vatom"], S.MVV2E, member=mem)
            assert np.array_equal(out, again) and out[6] == (s.n if mem is None else member.sum())
            assert np.all(np.abs(out - ref["sums"]) <= 1e-12 * ref["mag"]), np.abs(out - ref["sums"]) / ref["mag"]
            assert np.all(ref["mag"][:6] > 1.0)
            worst.append(float((np.abs(out - ref["sums"]) / ref["mag"]).max()))
        with capsys.disabled():
            print(f"70 304 atoms, heat current against fsum: worst |device - exact| / sum|term| {worst[0]:.2e} (all), {worst[1]:.2e} (a third)")
    finally:
        ctx.close()


def test_a_group_of_nobody():
    """a group bit carried by no atom: mdp_heatflux_sums gives eight zeros, the count among them"""
    s, v0 = _system("rebomos", 300.0)
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.set_group(np.ones(s.n + 1, dtype=np.int32), 0)
        d.compute(3, 5)
        out = ctx.heatflux_sums(group_bit=4)
        assert out.shape == (8,) and not out.any()
        assert not d.heatflux(group_bit=4).any() and ctx.heatflux_sums()[6] == s.n
    finally:
        ctx.close()
