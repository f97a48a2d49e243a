"""What the indenters and the tether springs compute, as hashes: positions, velocities and every state word at steps 0, 20,
40 and 200 of four short runs on the alloy cell of the tests without its silicon (fcc Al, a = 4.045 A, 6^3 cells, 864 atoms,
300 K: no three-body forces, whose float atomics would make two runs differ in the last bits), with the library
MDP_LIB_PATH names (default: this build).  Run it once per library and compare the two files: they must be identical.
  spring+indenter   resident: one spring on the integrate group next to a static sphere on every atom
  four-indenters    resident: two spheres, a plane and a cylinder on four group bits
  four-springs      resident: four springs on four group bits, two tether points moving, one with two dimensions left out
  host-linked       mdp_hnve_*: a moving and a static sphere, the host's atom order a shuffle, re-uploads every 50 steps
Reads at 20 find the final half deferred, the others done.  Neither the oracle nor any reference is used.
Usage: [MDP_LIB_PATH=lib.so] python profiles/postforce_stage/dump_states.py out.txt"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g   # noqa: E402

g.load_package()
import numpy as np   # noqa: E402
from lammps_plugins_amd.host import capi, resident, system as S   # noqa: E402

POT = os.path.join(ROOT, "tests", "golden", "potentials", "AlSi.aeam")
A0, DT, SKIN, NSTEPS, READS = 4.045, 0.001, 0.5, 200, (20, 40, 200)
GBIT, A_BIT, B_BIT, C_BIT = 2, 4, 8, 16
SPHERE = dict(shape="sphere", k=5.0, r=2.3, c=(3.5 * A0, 3.5 * A0, 3.5 * A0), bit=0)
MOVING = dict(shape="sphere", k=5.0, r=3.0584, c=(4.2549, 12.5983, 6.0378), vel=(-1.7802, -2.0251, 10.4168), bit=GBIT)
FOUR = [SPHERE, MOVING, dict(shape="plane", side="lo", dim=2, k=20.0, c=(0.0, 0.0, 2.5 * A0 + 0.15), bit=A_BIT),
        dict(shape="cylinder", side="out", dim=0, k=5.0, r=2.3, c=(0.0, 3.5 * A0, 3.5 * A0), vel=(0.0, 0.1, 0.0), bit=C_BIT)]


def system():
    af = capi.AeamFile(POT)
    s = S.fcc_cell(A0, 6, frac_type2=0.0, seed=92)
    s.mass[1:3] = af.mass[:2]
    by_tag = np.ones(s.n + 1, dtype=np.int32)
    t = np.arange(s.n + 1)
    by_tag[t % 3 != 0] |= GBIT                       # a third of the cell is held
    for bit, r in ((A_BIT, 1), (B_BIT, 2), (C_BIT, 4)):
        by_tag[(t % 3 != 0) & (t % 7 == r)] |= bit
    return af, s, S.gaussian_velocities(s, 300.0, seed=93), by_tag


def springs(s, by_tag):
    x = S.wrap(s.box, s.x)

    def sp(bit, k, off, r0=0.0, vel=(0.0, 0.0, 0.0)):
        l = (by_tag[s.tag] & bit) != 0
        m = s.mass[s.type][l]
        c0 = (m[:, None] * x[l]).sum(axis=0) / m.sum()
        return dict(k=k, r0=r0, c=tuple(None if o is None else float(c0[d] + o) for d, o in enumerate(off)), vel=vel, bit=bit)
    return [sp(GBIT, 25.0, (5.0, -3.0, 1.0)), sp(A_BIT, 40.0, (0.4, None, None), vel=(9.0, 0.0, 0.0)),
            sp(B_BIT, 40.0, (-0.5, 0.8, 0.3), r0=2.0), sp(C_BIT, 30.0, (None, 1.2, -0.6), vel=(0.0, 2.0, 2.0))]


def words(st):
    return np.concatenate([np.atleast_1d(np.asarray(st[w], dtype=np.float64)) for w in sorted(st)])


def resident_case(inds, sprs):
    af, s, v0, by_tag = system()
    ctx = capi.Context(0)
    try:
        tabs = af.build()
        ctx.aeam_set_tables(tabs)
        d = resident.DeviceDomain(ctx, capi.STYLE_AEAM, s, float(af.cut_table(tabs).max()) + SKIN, SKIN, None, v0=v0)
        d.set_group(by_tag, GBIT)
        d.track_images()
        d.compute(1, 0)
        if inds:
            d.indent(inds)
        if sprs:
            d.spring(sprs)

        def states():
            return [words(d.indent_state(k)) for k in range(len(inds))] + [words(d.spring_state(k)) for k in range(len(sprs))]
        out = {0: states()}
        for step in range(1, NSTEPS + 1):
            d.step(0, 0, rebuild="auto", defer_final=step not in READS or step == 20)
            if step in READS:
                st = states()
                d.flush()
                got = ctx.md_download(d.nlocal, want=("x", "v"))
                x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
                x[d.tags_local - 1], v[d.tags_local - 1] = got["x"], got["v"]
                out[step] = [x, v] + st
        return out
    finally:
        ctx.close()


def hostlinked_case():
    af, s, v0, by_tag = system()
    inds = [MOVING, SPHERE]
    perm = np.random.default_rng(17).permutation(s.n)
    type_p, tag_p = s.type[perm].copy(), s.tag[perm].copy()
    mask_p, gp = by_tag[tag_p], (by_tag[tag_p] & GBIT) != 0
    c = capi.Context(0)
    try:
        tabs = af.build()
        c.aeam_set_tables(tabs)
        c.aeam_device_lists(True)
        cut = float(af.cut_table(tabs).max()) + 1.0

        def upload(x, v):
            xa, type_all, tag_all, _, _, nloc, _ = S.with_ghosts(S.System(s.box, x.copy(), type_p, tag_p, s.mass), cut)
            c.set_atoms_host(nloc, xa, type_all, tag_all, 2, map_=None)
            c.set_skin(1.0)
            c.hnve_upload_v(v)

        def compute():
            eng, vir = C.c_double(0.0), np.zeros(6)
            c._ck(c.L.mdp_aeam_density_host(c.h, C.c_int(0), None, None, C.byref(eng), None))
            c._ck(c.L.mdp_aeam_force_host(c.h, C.c_int(0), C.c_int(0), None, None, C.byref(eng), capi._dp(vir), None, None))

        def read():
            st = [words(c.indent_state(k)) for k in range(2)]
            got = c.hnve_download(s.n, want=("x", "v"))
            x, v = np.zeros((s.n, 3)), np.zeros((s.n, 3))
            x[tag_p - 1], v[tag_p - 1] = got["x"], got["v"]
            return [x, v] + st
        c.hnve_setup(DT, S.FTM2V, s.mass)
        c.integrate_group(GBIT)
        c.set_box_host(s.box)
        upload(S.wrap(s.box, s.x)[perm].copy(), v0[perm])
        c.hnve_set_mask(mask_p)
        compute()
        c.indent_setup(inds)
        c.indent_run(0)
        out = {0: read()[2:]}
        for step in range(1, NSTEPS + 1):
            moved, late = c.hnve_initial()
            if moved or step % 50 == 0:
                got = c.hnve_download(s.n, want=("x", "v"))
                xw = S.wrap(s.box, got["x"])
                xw[~gp] = got["x"][~gp]
                upload(xw, got["v"])
                c.hnve_set_mask(mask_p)
            compute()
            c.hnve_final()
            if step in READS:
                out[step] = read()
        return out
    finally:
        c.close()


def main():
    af, s, v0, by_tag = system()
    sprs = springs(s, by_tag)
    cases = {"spring+indenter": lambda: resident_case([SPHERE], sprs[:1]), "four-indenters": lambda: resident_case(FOUR, []),
             "four-springs": lambda: resident_case([], sprs), "host-linked": hostlinked_case}
    lines = []
    for name, run in cases.items():
        out = run()
        for step in sorted(out):
            h = hashlib.sha256()
            for a in out[step]:
                h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
            # (the last state's first words in clear, so that a reader sees the stage acts)
            lines.append(f"{name} step {step}: {len(out[step])} arrays sha256 {h.hexdigest()}  last state {out[step][-1][:3].tolist()}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(sys.argv[1], "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
