"""GPU: image flags on the device (mdp_md_set_image: counted by the remap of every reneighbouring, carried through the
re-ordering and the migration), the unwrapped positions x + h . image and the mean-squared displacement measured with
them (mdp_msd_*, csrc/msd.hip), against tests/msdref.py -- velocity Verlet around the ORACLE with a wrapped x and an
integer image per atom, as LAMMPS keeps them."""
import math

import numpy as np
import pytest

from conftest import POT_AEAM, POT_REBOMOS
from lammps_plugins_amd.host import capi, resident, system as S
import mdref
import msdref

pytestmark = pytest.mark.gpu

XTOL = 1e-9      # A: the project's bound for positions against a host loop (tests/test_gpu_langevin_mdp.py)
MSD_RTOL = 1e-12  # a sum of n non-negative terms in any order is off by at most n 2^-53 relative: 2.6e-13 for n = 2 304


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


def _by_tag(n, tags, a):
    out = np.zeros((n,) + a.shape[1:], dtype=a.dtype)
    out[tags - 1] = a
    return out


def _state(d, n):
    tags = d.tags_local
    got = d.ctx.md_download(d.nlocal, want=("x", "v"))
    return dict(tags=tags.copy(), x=_by_tag(n, tags, got["x"]), v=_by_tag(n, tags, got["v"]),
                image=_by_tag(n, tags, d.images_local()), xu=_by_tag(n, tags, d.unwrapped_local()))


@pytest.mark.parametrize("style", ["rebomos", "aeam"])
def test_one_brick_unwraps_what_the_reference_unwraps(oracle, style, capsys):
    """300 K plus a drift of several hundred A/ps, the lists rebuilt every step: every atom leaves the box, some twice in
    one dimension (asserted on the reference's images); REBO-MoS in the sheared box, where the unwrap has the xy term.
    The device's unwrapped positions against the reference's, by tag and without any modulo of box vectors (a missed
    image is a whole box vector, > 10 A), and its image counts against the reference's integers.
    The test prints the measured deviations at every read.  Measured on an MI355X (bound 1e-9 A):
      rebomos, 1 152 atoms  step 20: |xu - reference| 1.42e-14 A, 0 atoms' images differ, |image| up to 1
                            step 40:                  1.78e-14 A, 0,                      |image| up to 2
      aeam, 864 atoms       step 25:                  7.11e-15 A, 0,                      |image| up to 1
                            step 50:                  2.13e-14 A, 0,                      |image| up to 2
    -- a few units in the last place of coordinates of tens of A: the device and the reference round alike."""
    s, v0, nsteps, ref = msdref.drift_reference(oracle, style, POT_REBOMOS, POT_AEAM)
    final = ref[nsteps][1]
    assert np.all(np.any(final != 0, axis=1)) and np.abs(final).max() >= 2      # (not vacuous)
    ctx, st, skin, cutghost, map_ = _context(style)
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.track_images()
        assert not d.images_local().any()
        d.compute(0, 0)
        for step in range(1, nsteps + 1):
            d.step(0, 0, rebuild=True)
            if step in ref:
                got = _state(d, s.n)
                dev = float(np.abs(got["xu"] - ref[step][2]).max())
                with capsys.disabled():
                    print(f"{style} {s.n} atoms, step {step}: |xu - reference| {dev:.2e} A, images "
                          f"{int((got['image'] != ref[step][1]).any(axis=1).sum())} atoms differ, |image| up to {int(np.abs(got['image']).max())}")
                assert dev < XTOL, (step, dev)
                assert np.array_equal(got["image"], ref[step][1]), step
                # the wrapped positions are the reference's too, and inside the box
                assert float(np.abs(got["x"] - ref[step][0]).max()) < XTOL
        assert d.builds == nsteps + 1
    finally:
        ctx.close()


# ---- the drift case of test_migration_keeps_the_noise (tests/test_gpu_langevin_mdp.py) without its thermostat: the
# (2, 2, 2) MoS2 replica, 2 304 atoms, 300 K plus (60, -45, 30) A/ps, 40 steps, reneighbourings forced every 5
MIG_DRIFT, MIG_STEPS, MIG_RENB, MIG_READS = (60.0, -45.0, 30.0), 40, 5, (20, 40)


def _mig_system():
    s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 2))
    v0 = S.gaussian_velocities(s, 300.0, seed=8) + np.array(MIG_DRIFT)
    vcap = float(np.sqrt((v0 ** 2).sum(axis=1)).max()) + 5.0 * np.sqrt(S.BOLTZ * 300.0 / (float(s.mass[1:3].min()) * S.MVV2E))
    assert int(0.3 * 2.0 / (vcap * 0.001)) >= MIG_RENB       # no atom moves 0.3 skin between two builds
    return s, v0


def _mig_run(s, v0, world, images, mask_by_tag=None):
    """the case on `world` bricks; images: track them (and measure the MSD of all atoms from the start).  Per rank: the
    states at the reads, the MSD values there, the migration records of every reneighbouring, atoms that left."""
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            out, left, records, at = {}, 0, {}, [0]
            tr = make_tr(ctx) if world > 1 else None
            if tr is not None:   # the migration records of a reneighbouring: what the 8-double exchange is handed to send
                plain_exchange = tr.exchange

                def exchange(send, send_counts, recv_counts, width, **kw):
                    if width == 8:
                        nrec = int(np.sum(send_counts))
                        records[at[0]] = send[:8 * nrec].cpu().numpy().reshape(nrec, 8).copy()
                    return plain_exchange(send, send_counts, recv_counts, width, **kw)
                tr.exchange = exchange
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, transport=tr)
            if mask_by_tag is not None:
                d.set_group(mask_by_tag, 0)
            if images:
                d.track_images()
                d.msd()
            d.compute(0, 0)
            for step in range(1, MIG_STEPS + 1):
                rb = step % MIG_RENB == 0
                at[0] = step
                d.step(0, 0, rebuild=rb)
                if rb:
                    left += ctx.dd_info()["left_last"]
                if step in MIG_READS:
                    tags = d.tags_local
                    got = ctx.md_download(d.nlocal, want=("x", "v"))
                    out[step] = dict(tags=tags.copy(), x=got["x"], v=got["v"])
                    if mask_by_tag is not None:
                        out[step]["mask"] = d.mask_local()[:, None]
                    if images:
                        out[step].update(image=d.images_local(), xu=d.unwrapped_local(), msd=d.msd_read(),
                                         msd_com=d.msd_read(com=True), msd_again=d.msd_read())
            return dict(out=out, left=left, records=records)
        finally:
            ctx.close()

    res = [rank_fn(0, None)] if world == 1 else resident.run_ranks(world, rank_fn)
    merged = {}
    for step in MIG_READS:
        m = dict(owner=np.zeros(s.n, dtype=int), seen=np.zeros(s.n, dtype=int))
        for k, r in enumerate(res):
            o = r["out"][step]
            m["owner"][o["tags"] - 1] = k
            m["seen"][o["tags"] - 1] += 1
            for key in ("x", "v", "image", "xu", "mask"):
                if key in o:
                    m.setdefault(key, np.zeros((s.n, o[key].shape[1]), dtype=o[key].dtype))[o["tags"] - 1] = o[key]
        for key in ("msd", "msd_com", "msd_again"):
            if images:
                assert all(np.array_equal(r["out"][step][key], res[0]["out"][step][key]) for r in res)   # every rank reads the same
                m[key] = res[0]["out"][step][key]
        assert np.all(m["seen"] == 1)
        merged[step] = m
    records = {step: np.concatenate([r["records"][step] for r in res]) for step in (res[0]["records"] if world > 1 else ()) if step > 0}
    return merged, sum(r["left"] for r in res), records


@pytest.fixture(scope="module")
def mig_reference(oracle):
    s, v0 = _mig_system()
    P = oracle.rebomos_params(POT_REBOMOS)
    reads = set(range(MIG_RENB, MIG_STEPS + 1, MIG_RENB))
    return s, v0, msdref.run(lambda sy: mdref.RebomosCPU(oracle, P, sy, skin=2.0), s, v0, MIG_STEPS, MIG_RENB, reads)


def _apart(msd):
    """how far the four values of two trajectories can differ whose positions differ by XTOL at the most: a component is a mean
    of squares, |mean (d + e)^2 - mean d^2| <= 2 sqrt(mean d^2) XTOL + XTOL^2 (Cauchy-Schwarz); the total is their sum"""
    c = 2.0 * np.sqrt(np.asarray(msd)[:3]) * XTOL + XTOL ** 2
    return np.array([c[0], c[1], c[2], c.sum()])


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def test_msd_values_are_the_sums_of_the_downloaded_displacements(capsys):
    """msd_read(), with and without com, over all 2 304 atoms and over a group of a third of them, against math.fsum over
    the displacements downloaded from the SAME device state: what is compared is the device's fixed-order sum with the
    exact one, so the bound is the summation's, 1e-12 relative.  Two reads of one state are bitwise equal.
    The test prints the measured deviations at every read.  Measured on an MI355X, after 40 steps (bound 1e-12):
      all 2 304 atoms  com no:  msd 10.454192 A^2, relative to fsum 1.70e-16;  com yes:  0.012720 A^2, 8.39e-15
      768 atoms        com no:      10.468061 A^2,                  2.74e-16;  com yes:  0.012826 A^2, 1.37e-14
    (com yes subtracts a shift of 3.2 A from each displacement before it squares it: the larger figure is that
    cancellation, relative to a value 800 times smaller)."""
    s, v0 = _mig_system()
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        mask = np.ones(s.n + 1, dtype=np.int32)
        mask[3::3] |= 2                                    # tags 3, 6, ...: a third of the atoms in group bit 2
        d.set_group(mask, 0)
        d.track_images()
        x0 = _by_tag(s.n, d.tags_local, d.unwrapped_local())
        d.compute(0, 0)
        for step in range(1, MIG_STEPS + 1):
            d.step(0, 0, rebuild=step % MIG_RENB == 0)
        tags = d.tags_local
        xu = _by_tag(s.n, tags, d.unwrapped_local())
        assert np.array_equal(_by_tag(s.n, tags, d.mask_local()[:, None])[:, 0], mask[1:])
        m = s.mass[s.type]
        for bit, sel in ((0, np.ones(s.n, dtype=bool)), (2, (mask[1:] & 2) != 0)):
            assert sel.sum() in (s.n, s.n // 3)
            d.msd(x0, group_bit=bit)
            for com in (False, True):
                got, again = d.msd_read(com=com), d.msd_read(com=com)
                want = msdref.msd_values(xu, x0, sel=sel, mass_per_atom=m, com=com)
                with capsys.disabled():
                    print(f"group bit {bit} ({int(sel.sum())} atoms), com {com}: msd {got[3]:.6f} A^2, relative to fsum {_rel(got, want):.2e}")
                assert got.tobytes() == again.tobytes()
                assert _rel(got, want) < MSD_RTOL, (bit, com, got, want)
            assert got[3] < 1.0 < d.msd_read()[3]          # (com yes took the drift of 0.04 ps x 81 A/ps out)
        d.msd_off()
        with pytest.raises(capi.MdpError, match="mdp_msd_setup not called"):
            ctx.msd_sums()
    finally:
        ctx.close()


def test_the_flag_migrates_with_its_atom(mig_reference, capsys):
    """8 bricks over the thread transport against the reference and against one brick: more than 10 atoms change owner;
    xu (1e-9 A, no modulo), image counts (exact) and the four MSD values.  The MSD values of the 8-brick state against
    fsum over that state's own displacements to the summation bound 1e-12; against the reference and the one-brick run --
    other trajectories, XTOL apart at the most -- to what XTOL does to a mean of squares (_apart): 2 sqrt(msd) XTOL + XTOL^2.
    A run whose contexts were never given an image packs records that hold type and tag alone and follows the same
    trajectory bit for bit as the run with images: tracking changes no coordinate.
    The test prints the measured deviations at every read.  Measured on an MI355X, 766 atoms leaving a brick in all:
      step 20: |xu - reference| 7.11e-15 A, |xu - one brick| 7.11e-15 A; msd  2.616519 A^2, relative to fsum of its own
               state 0, to the reference 1.37e-16, to one brick 0
      step 40: |xu - reference| 1.42e-14 A, |xu - one brick| 1.42e-14 A; msd 10.454192 A^2, relative to fsum of its own
               state 1.70e-16, to the reference 1.70e-16, to one brick 0
    and the images of no atom differ (bounds: 1e-9 A, 1e-12 relative, _apart = 1.1e-8 A^2 on the total at step 40)."""
    s, v0, ref = mig_reference
    one, _, _ = _mig_run(s, v0, 1, images=True)
    # the 8-brick run with images carries a mask too (bit 2 and the sign bit on every third tag, no group bit set: every atom
    # is integrated), so that type, the mask's 32 bits and iz share r[6] of the records that migrate
    mask = np.ones(s.n + 1, dtype=np.uint32)
    mask[3::3] |= 0x80000002
    mask = mask.view(np.int32)
    dev, left, rec = _mig_run(s, v0, 8, images=True, mask_by_tag=mask)
    plain, left_plain, rec_plain = _mig_run(s, v0, 8, images=False)
    assert left > 10 and left == left_plain, (left, left_plain)
    assert len(set(dev[MIG_READS[-1]]["owner"])) == 8
    assert (dev[MIG_READS[0]]["owner"] != dev[MIG_READS[-1]]["owner"]).sum() >= 3
    x0 = ref[0][2]
    crossed = 0
    for step in MIG_READS:
        g, o, (xr, ir, xur, vr) = dev[step], one[step], ref[step]
        dx_ref, dx_one = float(np.abs(g["xu"] - xur).max()), float(np.abs(g["xu"] - o["xu"]).max())
        own = msdref.msd_values(g["xu"], x0)
        want = msdref.msd_values(xur, x0)
        with capsys.disabled():
            print(f"step {step}: {left} left in all; |xu - reference| {dx_ref:.2e} A, |xu - one brick| {dx_one:.2e} A; msd {g['msd'][3]:.6f} A^2, "
                  f"relative to fsum of its own state {_rel(g['msd'], own):.2e}, to the reference {_rel(g['msd'], want):.2e}, "
                  f"to one brick {_rel(g['msd'], o['msd']):.2e}")
        assert dx_ref < XTOL and dx_one < XTOL
        assert np.array_equal(g["image"], ir) and np.array_equal(o["image"], ir)
        assert np.array_equal(g["mask"][:, 0], mask[1:])      # the mask arrived with its atom, sign bit and all
        crossed += int(np.any(ir != 0, axis=1).sum())
        assert g["msd"].tobytes() == g["msd_again"].tobytes()
        assert _rel(g["msd"], own) < MSD_RTOL
        m = s.mass[s.type]
        assert _rel(g["msd_com"], msdref.msd_values(g["xu"], x0, mass_per_atom=m, com=True)) < MSD_RTOL
        for other in (want, o["msd"]):
            assert np.all(np.abs(g["msd"] - other) <= _apart(other))
        for other in (msdref.msd_values(xur, x0, mass_per_atom=m, com=True), o["msd_com"]):
            assert np.all(np.abs(g["msd_com"] - other) <= 2.0 * _apart(other))   # (the centre of mass moves by XTOL at the most too)
        # tracking images changes no coordinate: the run without them is the same trajectory, bit for bit
        assert g["x"].tobytes() == plain[step]["x"].tobytes() and g["v"].tobytes() == plain[step]["v"].tobytes()
    assert crossed > 0                                      # some atoms did leave the box
    # the migration records.  Without an image: {x, v, type, tag}, as they always were; with one the same six coordinates,
    # the image in the upper bits of the last two words, above the mask in r[6]
    assert sorted(rec) == sorted(rec_plain) == list(range(MIG_RENB, MIG_STEPS + 1, MIG_RENB))
    carried = 0
    for step in sorted(rec):
        a, b = rec_plain[step], rec[step]
        assert a.shape == b.shape
        tag_a, tag_b = a[:, 7].astype(np.int64), b[:, 7].astype(np.int64) % 2 ** 31
        a, b, tag_a, tag_b = a[np.argsort(tag_a)], b[np.argsort(tag_b)], np.sort(tag_a), np.sort(tag_b)
        assert np.array_equal(tag_a, tag_b)
        assert np.array_equal(a[:, 6], s.type[tag_a - 1].astype(np.float64)) and np.array_equal(a[:, 7], tag_a.astype(np.float64))
        assert a[:, :6].tobytes() == b[:, :6].tobytes()
        w6, w7 = b[:, 6].astype(np.int64), b[:, 7].astype(np.int64)
        assert np.array_equal(w6 % 64, s.type[tag_b - 1])
        assert np.array_equal((w6 >> 6) & 0xFFFFFFFF, mask.view(np.uint32)[tag_b].astype(np.int64))
        image = np.stack([(w7 >> 31) & 1023, (w7 >> 41) & 1023, w6 >> 38], axis=1) - 512
        assert np.array_equal(image, ref[step][1][tag_b - 1]), step
        carried += int(np.any(image != 0, axis=1).sum())
    assert carried > 0                                      # a non-zero flag did travel
    assert any((rec[step][:, 6].astype(np.int64) >> 6 & 0x80000000).any() for step in rec)   # ... and a mask with its sign bit


def test_refusals():
    s = S.rebomos_bulk_cell()
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        x0 = np.zeros((s.n, 3))
        for call in (lambda: ctx.msd_setup(s.n, x0), lambda: ctx.md_download_unwrapped(s.n)):
            with pytest.raises(capi.MdpError, match=r"no image set \(mdp_md_set_image\)"):
                call()
        with pytest.raises(capi.MdpError, match="no image set"):
            ctx.md_download_int("image", s.n)
        d.track_images()
        with pytest.raises(capi.MdpError, match="mdp_msd_setup not called"):
            ctx.msd_sums()
        with pytest.raises(capi.MdpError, match=r"a group is set but no mask covers the current atoms \(mdp_md_set_mask\)"):
            ctx.msd_setup(s.n, x0, groupbit=2)
        with pytest.raises(capi.MdpError, match="need ntag = the 288 owned atoms"):
            ctx.msd_setup(s.n + 1, None)
        ctx.msd_setup(s.n - 1, x0[:-1])                    # an owned atom whose tag has no origin
        with pytest.raises(capi.MdpError, match="tag outside 1 .. 287"):
            ctx.msd_sums()
        ctx.msd_setup(s.n, None)
        assert not ctx.msd_sums()[:3].any() and ctx.msd_sums()[3] == s.n
        ctx.md_set_image(None)                             # withdrawn: the measurement has nothing to unwrap with
        with pytest.raises(capi.MdpError, match="no image set"):
            ctx.msd_sums()
    finally:
        ctx.close()
    # without mdp_dd_setup: a resident context that holds an image
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        cfg = capi.MdConfig()
        cfg.style, cfg.nlocal, cfg.nghost, cfg.ntypes = st, s.n, 0, 2
        cfg.skin, cfg.dt, cfg.ftm2v, cfg.mvv2e, cfg.nghost_self = skin, 0.001, S.FTM2V, S.MVV2E, 0
        for k in range(3):
            cfg.bbox_lo[k], cfg.bbox_hi[k] = -30.0, 60.0
        e3, e1 = np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
        ctx.md_setup(cfg, s.x, np.zeros_like(s.x), s.type, s.tag, s.mass, map_, e1, e3, e1, e1)
        ctx.md_set_image(np.full(s.n, resident.IMAGE0, dtype=np.int32))
        assert np.array_equal(ctx.md_download_int("image", s.n), np.full(s.n, resident.IMAGE0))
        with pytest.raises(capi.MdpError, match="mdp_dd_setup not called"):
            ctx.msd_setup(s.n, np.zeros((s.n, 3)))
        with pytest.raises(capi.MdpError, match="mdp_dd_setup not called"):
            ctx.md_download_unwrapped(s.n)
    finally:
        ctx.close()

    # origins from the current positions on a brick of several ranks: an arrival's origin would be unknown
    def rank_fn(r, make_tr):
        ctx, st, skin, cutghost, map_ = _context("rebomos")
        try:
            d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, transport=make_tr(ctx))
            d.track_images()
            try:
                ctx.msd_setup(d.nlocal, None)
            except capi.MdpError as e:
                return str(e)
            return "accepted"
        finally:
            ctx.close()

    for msg in resident.run_ranks(2, rank_fn):
        assert "one rank only" in msg and "brick of 2 ranks" in msg, msg


# ---- the slots the runs above leave empty: more than 256 slots for mdp_slot_total_kernel<9>, the xz and yz terms of the
# unwrap in msd.hip's own kernels, a group of nobody
@pytest.fixture(scope="module")
def big():
    """70 304 aluminium atoms (fcc 26^3, as the indenter's second-trip test): 275 blocks.  Built once for this module."""
    s = S.fcc_cell(4.045, 26)
    s.mass[1:3] = capi.AeamFile(POT_AEAM).mass[:2]
    assert s.n == 70304 and -(-s.n // 256) == 275 and s.n % 256 == 160
    return s


def test_the_slot_sums_second_trip_against_fsum(big, capsys):
    """275 slots: mdp_slot_sum_256<9> takes a second trip.  Random images of -2 .. 2, origins passed by tag and displaced from
    the unwrapped positions by a known random vector per atom (about 2 A), no step taken.  The unwrapped positions against
    msdref.unwrap; the eight sums against math.fsum over the terms of the downloaded state.  Any order of adding n terms
    stays within n 2^-53 = 7.8e-12 of the sum of their magnitudes; asked here is the 1e-12 of the indenter's second-trip
    test (STOL, tests/test_gpu_indent_mdp.py), which a fixed tree meets with room."""
    s = big
    rng = np.random.default_rng(88)
    img = rng.integers(-2, 3, (s.n, 3))
    disp = rng.normal(0.0, 2.0, (s.n, 3))
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=np.zeros((s.n, 3)))
        assert -(-d.nlocal // 256) > 256                                   # the premise: more slots than lanes
        d.track_images(resident.image_pack(img))
        got = _state(d, s.n)
        assert np.array_equal(got["image"], img)
        want = msdref.unwrap(s.box, got["x"], img)
        assert np.abs(got["xu"] - want).max() <= 8 * 2.0 ** -53 * (np.abs(got["x"]).max() + 2 * s.box.prd.max())
        x0 = got["xu"] - disp
        shift = np.array([0.3, -0.2, 0.1])
        sums = {}
        for bit, sel in ((0, np.ones(s.n, dtype=bool)), (2, s.tag % 3 == 0)):
            if bit:
                mask = np.ones(s.n + 1, dtype=np.int32)
                mask[1:] |= 2 * sel.astype(np.int32)
                d.set_group(mask, 0)
            ctx.msd_setup(s.n, x0, bit)
            for sh in (None, shift):
                out, again = ctx.msd_sums(sh), ctx.msd_sums(sh)
                assert out.tobytes() == again.tobytes()
                dd = (got["xu"][sel] - x0[sel]) - (0.0 if sh is None else sh)
                m = s.mass[s.type][sel]
                cols = [dd[:, 0] ** 2, dd[:, 1] ** 2, dd[:, 2] ** 2, np.ones(len(m)), m * got["xu"][sel][:, 0], m * got["xu"][sel][:, 1],
                        m * got["xu"][sel][:, 2], m]
                ref = np.array([math.fsum(c) for c in cols])
                mag = np.array([math.fsum(np.abs(c)) for c in cols])
                sums[(bit, sh is None)] = float((np.abs(out - ref) / mag).max())
                assert out[3] == sel.sum() and np.all(np.abs(out - ref) <= 1e-12 * mag), (bit, np.abs(out - ref) / mag)
                assert out[:3].min() > 2.0 * sel.sum()                     # (the displacements are there: about 4 A^2 each)
        with capsys.disabled():
            print("70 304 atoms, msd sums against fsum, worst relative to the terms' magnitudes: "
                  + ", ".join(f"bit {b} shift {not p}: {w:.2e}" for (b, p), w in sums.items()))
    finally:
        ctx.close()


def test_a_box_with_all_three_tilts(capsys):
    """mdp_unwrap's xz and yz terms through msd.hip's own kernels: the 864-atom alloy sheared into the box of
    test_the_centre_of_mass_in_a_cell_sheared_in_xz_and_yz (tests/test_gpu_spring_mdp.py), 300 K plus a drift that changes
    images in x, y and z within 30 steps (lists rebuilt every step).  Origins from the current positions at the start
    (msd_origin_kernel), unwrapped_local (msd_unwrap_kernel) and the sums (msd_partial_kernel) against msdref in that box.
    Not vacuous: unwrapped with the box stripped of xz and yz, the positions are tenths of an A elsewhere."""
    af = capi.AeamFile(POT_AEAM)
    s0 = S.fcc_cell(4.045, 6, frac_type2=0.05, seed=92)
    s0.mass[1:3] = af.mass[:2]
    box = S.Box(s0.box.lo.copy(), s0.box.prd.copy(), np.array([0.35, -0.45, 0.25]))
    s = S.System(box, np.ascontiguousarray(box.lamda2x(s0.box.x2lamda(s0.x))), s0.type, s0.tag, s0.mass)
    flat = S.Box(box.lo, box.prd, np.array([0.35, 0.0, 0.0]))
    v0 = S.gaussian_velocities(s, 300.0, seed=3) + np.array([500.0, -400.0, 300.0])
    ctx, st, skin, cutghost, map_ = _context("aeam")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0)
        d.track_images()
        x0 = _by_tag(s.n, d.tags_local, d.unwrapped_local())
        d.msd()                                                            # origins from the current positions
        d.compute(0, 0)
        for _ in range(30):
            d.step(0, 0, rebuild=True)
        got = _state(d, s.n)
        assert all((got["image"][:, k] != 0).sum() > s.n // 4 for k in range(3))
        want = msdref.unwrap(s.box, got["x"], got["image"])
        bound = 8 * 2.0 ** -53 * (np.abs(got["x"]) + S.mul_upper(np.abs(got["image"]).astype(float), np.abs(s.box.h)))
        assert np.all(np.abs(got["xu"] - want) <= bound)
        moved = np.abs(msdref.unwrap(flat, got["x"], got["image"]) - want)
        assert moved[:, 0].max() > 0.4 and moved[:, 1].max() > 0.2           # (xz and yz do matter to it)
        m = s.mass[s.type]
        for com in (False, True):
            val = d.msd_read(com=com)
            ref = msdref.msd_values(got["xu"], x0, mass_per_atom=m, com=com)
            with capsys.disabled():
                print(f"all three tilts, com {com}: msd {val[3]:.6f} A^2, relative to fsum {_rel(val, ref):.2e}")
            assert _rel(val, ref) < MSD_RTOL, (com, val, ref)
        assert d.msd_read()[3] > 100.0 > d.msd_read(com=True)[3]
        wrong = msdref.msd_values(msdref.unwrap(flat, got["x"], got["image"]), x0)
        assert _rel(d.msd_read(), wrong) > 1e-6
    finally:
        ctx.close()


def test_a_group_of_nobody():
    """a group bit carried by no atom: mdp_msd_sums gives eight zeros, the count among them"""
    s = S.rebomos_bulk_cell()
    ctx, st, skin, cutghost, map_ = _context("rebomos")
    try:
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_)
        d.set_group(np.ones(s.n + 1, dtype=np.int32), 0)
        d.track_images()
        ctx.msd_setup(s.n, np.zeros((s.n, 3)), groupbit=4)
        for shift in (None, np.array([1.0, 2.0, 3.0])):
            out = ctx.msd_sums(shift)
            assert out.shape == (8,) and not out.any()
        ctx.msd_setup(s.n, np.zeros((s.n, 3)))
        assert ctx.msd_sums()[3] == s.n
    finally:
        ctx.close()
