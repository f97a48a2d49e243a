"""One-off for the change that gave compute adf/mdp, coord/atom/mdp and centro/atom/mdp one stencil walk (csrc/measure_walk.h): the
four neighbour reads return the same bits from the PARENT commit's library and from this build, on the same device state.
Both libraries are loaded into one process; the run is this build's, and every state is read through the parent's library and
then through this build's on the SAME context (the two have one mdp_ctx layout: the change touches no field of it).  Two
processes do not do: the alloy's states are not reproduced bit for bit from process to process -- with either library alone
centro at the shell's limit returns a different last bit in a few atoms in every process, the owned positions and the number of
list builds being equal -- so hashes from two processes say nothing about the kernels.  The states:
  * the 864-atom alloy and the 1 152-atom MoS2 cell of tests/test_gpu_struct_mdp.py::test_one_brick at 300 K and 2 500 K, after
    their 25 steps, and the alloy with free z at 2 500 K of test_a_non_periodic_dimension;
  * a group of four atoms in five, by tag (a member table for rdf and adf, the mask bit for coord and centro);
  * rdf at the ghost shell's limit with the columns * *, 1 1, 1 2, 2 1, 2 2; adf with a first-shell and a wide triple; coord with the
    columns *, 1, 2; centro as test_one_brick sets it up;
  * every read with MDP_MEASURE_GRID unset and 1.
The SHA-256 of every returned array goes to identity.txt, parent and this build side by side; exit status 1 if a row differs.
Usage: python profiles/measure_walk/identity.py --parent-lib PATH [identity.txt]"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden", "potentials")
STATES = [("aeam", 300.0, False), ("aeam", 2500.0, False), ("rebomos", 300.0, False), ("rebomos", 2500.0, False), ("aeam", 2500.0, True)]
GBIT = 2
COORD_RC = {"rebomos": 2.8, "aeam": 3.5}
CENTRO = {"rebomos": (6, 4.0), "aeam": (12, None)}


def child(parent_path):
    sys.path.insert(0, ROOT)
    import ctypes
    import __graft_entry__ as g
    g.load_package()
    import numpy as np
    from lammps_plugins_amd.host import capi, resident, system as S
    capi.lib()                                             # this build's, before the parent's: torch's HIP runtime serves both
    parent = ctypes.CDLL(parent_path)
    parent.mdp_last_error.restype = ctypes.c_char_p
    parent.mdp_md_ptr.restype = ctypes.c_void_p
    parent.mdp_device_bytes.restype = ctypes.c_double

    def sha(name, a):
        a = np.ascontiguousarray(a)
        print(f"HASH {name} {a.dtype}[{'x'.join(str(k) for k in a.shape)}] {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)

    for style, temp, free_z in STATES:
        ctx = capi.Context(0)
        if style == "rebomos":
            p = capi.read_rebomos_file(os.path.join(GOLD, "MoS.REBO.set5b"))
            ctx.rebomos_set_params(p)
            st, skin, cutghost, map_ = capi.STYLE_REBOMOS, 2.0, 3.0 * p.rcmax[0][0] + 2.0, [0, 0, 1]
            s = S.replicate(S.rebomos_bulk_cell(), (2, 2, 1))
        else:
            af = capi.AeamFile(os.path.join(GOLD, "AlSi.aeam"))
            tabs = af.build()
            ctx.aeam_set_tables(tabs)
            st, skin, cutghost, map_ = capi.STYLE_AEAM, 1.0, float(af.cut_table(tabs).max()) + 1.0, None
            s = S.fcc_cell(4.045, 6, frac_type2=0.05, seed=92)
            s.mass[1:3] = af.mass[:2]
        v0 = S.gaussian_velocities(s, temp, seed=3)
        d = resident.DeviceDomain(ctx, st, s, cutghost, skin, map_, v0=v0, **({"nonperiodic": (0, 0, 1)} if free_z else {}))
        member = np.arange(1, s.n + 1) % 5 != 0
        mask = np.ones(s.n + 1, dtype=np.int32)
        mask[1:][member] |= GBIT
        d.set_group(mask, 1)
        limit = cutghost - skin
        nnn, rc = CENTRO[style]
        def setups():
            d.rdf(50, limit, [((1, 2), (1, 2)), (1, 1), (1, 2), (2, 1), (2, 2)], member_by_tag=member)
            d.adf(45, [((1, 2), (1, 2), (1, 2), 0.0, COORD_RC[style], 0.0, COORD_RC[style]), (1, (1, 2), 2, 0.0, 4.0, 1.0, 4.0)], member_by_tag=member)
            d.coord(COORD_RC[style], [(1, 2), (1, 1), (2, 2)], group_bit=GBIT)
            d.centro(nnn, rc, group_bit=GBIT)

        setups()
        d.compute(0, 0)
        for _ in range(25):
            d.step(0, 0, rebuild="auto")
        d.flush()                                          # nothing of the run is left for the parent's library to complete
        state = f"{style}_{temp:.0f}K{'_free_z' if free_z else ''}"
        for name, L in (("parent", parent), ("this", ctx.L)):
            ctx.L = L
            setups()
            for knob in (None, "1"):
                os.environ.pop("MDP_MEASURE_GRID", None)
                if knob:
                    os.environ["MDP_MEASURE_GRID"] = knob
                key = f"{name} {state}.grid_{knob or 'unset'}"
                for what, a in zip(("hist", "icount", "jcount", "dup"), d.rdf_read()):
                    sha(f"{key}.rdf.{what}", a)
                for what, a in zip(("hist", "icount"), d.adf_read()):
                    sha(f"{key}.adf.{what}", a)
                tags, val = d.coord_read()
                sha(f"{key}.coord.tags", tags)
                sha(f"{key}.coord.values", val)
                tags, val = d.centro_read()
                sha(f"{key}.centro.values", val)
                sha(f"{key}.centro.few", np.array([ctx.centro_info()["few"]], dtype=np.int64))
        os.environ.pop("MDP_MEASURE_GRID", None)
        ctx.close()


def main():
    args = sys.argv[1:]
    parent = os.path.abspath(args[args.index("--parent-lib") + 1])
    out_path = next((a for a in args if a.endswith(".txt")), os.path.join(os.path.dirname(os.path.abspath(__file__)), "identity.txt"))
    env = dict(os.environ)
    env.pop("MDP_LIB_PATH", None)
    env.pop("MDP_MEASURE_GRID", None)
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", parent], capture_output=True, text=True, env=env)
    rows = [l.split()[1:] for l in p.stdout.splitlines() if l.startswith("HASH ")]
    if p.returncode != 0 or not rows:
        print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
        print(f"exit status {p.returncode}; stopping", file=sys.stderr)
        sys.exit(2)
    cols = [{r[1]: r[2:] for r in rows if r[0] == lib} for lib in ("parent", "this")]
    assert list(cols[0]) == list(cols[1]) and [v[0] for v in cols[0].values()] == [v[0] for v in cols[1].values()]
    differ = 0
    with open(out_path, "w") as f:
        f.write("# array, dtype and shape, SHA-256 through the parent commit's library, SHA-256 through this build, on one device state\n")
        f.write("# this build: lammps-plugins_amd/libmdpair_hip.so as it stood beside these sources (SHA-256; a later edit of one shows here):\n")
        for name in ("measure_walk.h", "adf.hip", "coord.hip", "centro.hip", "rdf.hip", "measure_bin.hip", "mdp_common.h"):
            with open(os.path.join(ROOT, "lammps-plugins_amd", "csrc", name), "rb") as src:
                f.write(f"#   csrc/{name} {hashlib.sha256(src.read()).hexdigest()}\n")
        for k, (shape, a) in cols[0].items():
            b = cols[1][k][1]
            differ += a != b
            f.write(f"{k} {shape} {a} {b}{'' if a == b else '  DIFFERENT'}\n")
        f.write(f"# {len(cols[0])} arrays, {differ} differ\n")
    print(f"{len(cols[0])} arrays, {differ} differ -> {out_path}")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    child(sys.argv[2]) if sys.argv[1:2] == ["--child"] else main()
