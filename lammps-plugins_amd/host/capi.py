"""ctypes binding of libmdpair_hip.so (include/mdpair_hip.h).  Python never computes forces itself:
every call here lands in the HIP kernels, and loading fails loudly when the library is missing."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libmdpair_hip.so")

D22 = (C.c_double * 2) * 2


class RebomosParams(C.Structure):
    """mirror of mdp_rebomos_params"""
    _fields_ = [(n, D22) for n in ("rcmin", "rcmax", "rcmaxsq", "Q", "alpha", "A", "BIJc", "Beta")] + [
        ("b", (C.c_double * 2) * 7), ("bg", (C.c_double * 2) * 7), ("a", (C.c_double * 2) * 4)] + [
        (n, D22) for n in ("rcLJmin", "rcLJmax", "epsilon", "sigma", "lj1", "lj2", "lj3", "lj4")]


class AeamTables(C.Structure):
    """mirror of mdp_aeam_tables"""
    _fields_ = [("ntypes", C.c_int), ("nelements", C.c_int), ("nnonangular", C.c_int),
                ("nrhomax", C.c_int), ("nrmax", C.c_int), ("nfrho", C.c_int), ("nrhor", C.c_int), ("nz2r", C.c_int),
                ("nrho", C.POINTER(C.c_int)), ("drho", C.POINTER(C.c_double)),
                ("nr", C.POINTER(C.c_int)), ("dr", C.POINTER(C.c_double)), ("cut", C.POINTER(C.c_double)),
                ("type2frho", C.POINTER(C.c_int)), ("type2rhor", C.POINTER(C.c_int)), ("type2z2r", C.POINTER(C.c_int)),
                ("frho_spline", C.POINTER(C.c_double)), ("rhor_spline", C.POINTER(C.c_double)),
                ("z2r_spline", C.POINTER(C.c_double))]


class MdConfig(C.Structure):
    """mirror of mdp_md_config"""
    _fields_ = [("style", C.c_int), ("nlocal", C.c_int), ("nghost", C.c_int), ("ntypes", C.c_int),
                ("skin", C.c_double), ("dt", C.c_double), ("ftm2v", C.c_double), ("mvv2e", C.c_double),
                ("bbox_lo", C.c_double * 3), ("bbox_hi", C.c_double * 3), ("nghost_self", C.c_int),
                ("master_list", C.c_int)]


class DdConfig(C.Structure):
    """mirror of mdp_dd_config"""
    _fields_ = [("boxlo", C.c_double * 3), ("h", C.c_double * 6), ("procgrid", C.c_int * 3), ("rank", C.c_int),
                ("cutghost", C.c_double), ("self_remote", C.c_int), ("nonperiodic", C.c_int * 3)]


class NhcConfig(C.Structure):
    """mirror of mdp_nhc_config"""
    _fields_ = [("t_start", C.c_double), ("t_stop", C.c_double), ("t_period", C.c_double), ("tchain", C.c_int),
                ("tloop", C.c_int), ("drag", C.c_double), ("nf", C.c_double), ("boltz", C.c_double),
                ("mvv2e", C.c_double)]


NHC_STATE_LEN, NHC_MAXCHAIN = 28, 8


class LangevinConfig(C.Structure):
    """mirror of mdp_langevin_config"""
    _fields_ = [("t_start", C.c_double), ("t_stop", C.c_double), ("t_period", C.c_double), ("seed", C.c_int),
                ("zero", C.c_int), ("tally", C.c_int), ("boltz", C.c_double), ("mvv2e", C.c_double),
                ("ratio", C.c_double * 16), ("natoms", C.c_longlong)]
class HeatConfig(C.Structure):
    """mirror of mdp_heat_config"""
    _fields_ = [("eflux", C.c_double), ("nevery", C.c_int), ("mvv2e", C.c_double)]
HEAT_MAXSRC, HEAT_STATE_LEN = 4, 8   # MDP_HEAT_MAXSRC, MDP_HEAT_STATE_LEN of include/mdpair_hip.h
class IndentConfig(C.Structure):
    """mirror of mdp_indent_config"""
    _fields_ = [("shape", C.c_int), ("dim", C.c_int), ("side", C.c_int), ("k", C.c_double), ("c", C.c_double * 3),
                ("r", C.c_double), ("vel", C.c_double * 3)]
INDENT_MAX, INDENT_STATE_LEN = 4, 10   # MDP_INDENT_MAX, MDP_INDENT_STATE_LEN of include/mdpair_hip.h
INDENT_SHAPES = {"sphere": 0, "cylinder": 1, "plane": 2}
INDENT_SIDES = {"out": 0, "in": 1, "lo": 0, "hi": 1}
class SpringConfig(C.Structure):
    """mirror of mdp_spring_config"""
    _fields_ = [("k", C.c_double), ("r0", C.c_double), ("c", C.c_double * 3), ("use", C.c_int * 3), ("vel", C.c_double * 3)]
SPRING_MAX, SPRING_STATE_LEN = 4, 16   # MDP_SPRING_MAX, MDP_SPRING_STATE_LEN of include/mdpair_hip.h
class GforceConfig(C.Structure):
    """mirror of mdp_gforce_config"""
    _fields_ = [("kind", C.c_int), ("use", C.c_int * 3), ("f", C.c_double * 3)]
GFORCE_MAX, GFORCE_STATE_LEN = 4, 10   # MDP_GFORCE_MAX, MDP_GFORCE_STATE_LEN of include/mdpair_hip.h
GFORCE_KINDS = {"set": 0, "add": 1, "ave": 2}
class FireConfig(C.Structure):
    _fields_ = [("etol", C.c_double), ("ftol", C.c_double), ("maxiter", C.c_longlong), ("maxeval", C.c_longlong),
                ("dmax", C.c_double), ("tmax", C.c_double), ("tmin", C.c_double), ("delaystep", C.c_int),
                ("dtgrow", C.c_double), ("dtshrink", C.c_double), ("alpha0", C.c_double), ("alphashrink", C.c_double),
                ("halfstepback", C.c_int), ("initialdelay", C.c_int)]
FIRE_STATE_LEN = 21
FIRE_STOP = {0: "running", 1: "force tolerance", 2: "energy tolerance", 3: "max iterations", 4: "max force evaluations"}
FIRE_DEFAULTS = dict(dmax=0.1, tmax=10.0, tmin=0.02, delaystep=20, dtgrow=1.1, dtshrink=0.5, alpha0=0.25,
                     alphashrink=0.99, halfstepback=True, initialdelay=True)   # LAMMPS min_modify defaults for fire
BOLTZ_METAL = 8.617343e-5    # force->boltz, metal units
LANGEVIN_MAXBATH = 4         # MDP_LANGEVIN_MAXBATH of include/mdpair_hip.h


STYLE_REBOMOS, STYLE_AEAM = 1, 2
PROFILE_W = 5                # MDP_PROFILE_W of include/mdpair_hip.h
PROFILE_MAXBINS = 1 << 20
ADF_DEGREE, ADF_RADIAN, ADF_COSINE = 0, 1, 2     # MDP_ADF_* of include/mdpair_hip.h
ADF_ORDINATES = dict(degree=ADF_DEGREE, radian=ADF_RADIAN, cosine=ADF_COSINE)
ADF_MAXNEIGH = 128           # MDP_ADF_MAXNEIGH: the short list of a wave, of adf.hip and centro.hip
COORD_MAXCOL, CENTRO_MAXN = 32, 64               # MDP_COORD_MAXCOL, MDP_CENTRO_MAXN
CENTRO_LATTICE = dict(fcc=12, bcc=8)
CNA_MAXNEAR = 16             # MDP_CNA_MAXNEAR: the short list of a wave of cna.hip
CNA_FCC, CNA_HCP, CNA_BCC, CNA_ICO, CNA_OTHER = 1, 2, 3, 4, 5

EXPORTS = [
    "mdp_abi_version", "mdp_device_count", "mdp_create", "mdp_destroy", "mdp_last_error", "mdp_set_stream",
    "mdp_sync", "mdp_rebomos_set_params", "mdp_rebomos_read_file", "mdp_rebomos_params_from_scalars",
    "mdp_aeam_set_tables", "mdp_aeam_file_read", "mdp_aeam_file_info", "mdp_aeam_file_build", "mdp_aeam_file_free", "mdp_set_atoms_host", "mdp_set_positions_host",
    "mdp_set_box_host", "mdp_host_ghosts_derived",
    "mdp_set_neighbors_host", "mdp_set_skin", "mdp_set_neighbors_csr_host", "mdp_rebomos_compute_host", "mdp_aeam_density_host",
    "mdp_aeam_force_host", "mdp_md_setup", "mdp_md_build_neighbors", "mdp_md_initial_integrate",
    "mdp_md_final_integrate", "mdp_md_final_initial_integrate", "mdp_md_compute", "mdp_md_compute_begin", "mdp_md_compute_end", "mdp_md_pack_x", "mdp_md_unpack_x", "mdp_md_pack_scalar",
    "mdp_md_unpack_scalar", "mdp_md_pack_ghost_f", "mdp_md_unpack_add_f", "mdp_md_fold_self_ghost_f",
    "mdp_md_aeam_density", "mdp_md_aeam_force", "mdp_md_thermo", "mdp_md_download", "mdp_md_upload_x", "mdp_md_ptr",
    "mdp_md_neighbor_stats", "mdp_md_class_stats", "mdp_md_prune_stats", "mdp_hnve_setup", "mdp_hnve_off", "mdp_hnve_upload_v",
    "mdp_hnve_initial", "mdp_hnve_final", "mdp_hnve_download", "mdp_rebomos_list_info", "mdp_set_timing", "mdp_get_timing",
    "mdp_device_bytes", "mdp_host_release", "mdp_rebomos_check_host_list",
    "mdp_dd_setup", "mdp_dd_reneighbor", "mdp_dd_migrate_begin", "mdp_dd_migrate_pack", "mdp_dd_migrate_end",
    "mdp_dd_borders_begin", "mdp_dd_borders_pack", "mdp_dd_borders_end", "mdp_dd_info", "mdp_dd_forward_pack",
    "mdp_dd_forward_unpack", "mdp_dd_forward_scalar_pack", "mdp_dd_forward_scalar_unpack", "mdp_dd_reverse_pack",
    "mdp_dd_reverse_unpack", "mdp_md_moved_async", "mdp_md_integrate_check", "mdp_md_download_int", "mdp_md_download_x_all",
    "mdp_dd_comm_unique_id", "mdp_dd_comm_library", "mdp_dd_comm_init", "mdp_dd_comm_destroy", "mdp_dd_comm_reneighbor",
    "mdp_dd_comm_forward_begin", "mdp_dd_comm_forward_end", "mdp_dd_comm_forward_scalar", "mdp_dd_comm_reverse",
    "mdp_dd_comm_allreduce", "mdp_dd_comm_step_begin", "mdp_dd_comm_step_end", "mdp_dd_comm_step_info", "mdp_aeam_device_lists", "mdp_rebomos_host_list", "mdp_aeam_check_host_list",
    "mdp_md_defer_final", "mdp_md_list_state", "mdp_md_aeam_force_begin", "mdp_md_aeam_state", "mdp_dd_comm_aeam_exchange_begin", "mdp_dd_comm_aeam_exchange_end",
    "mdp_nhc_setup", "mdp_nhc_run", "mdp_nhc_state", "mdp_nhc_set_state", "mdp_nhc_off",
    "mdp_langevin_setup", "mdp_langevin_run", "mdp_langevin_tally", "mdp_langevin_off",
    "mdp_langevin_baths", "mdp_langevin_tally_bath",
    "mdp_fire_setup", "mdp_fire_iterate", "mdp_fire_state", "mdp_fire_off",
    "mdp_md_set_mask", "mdp_hnve_set_mask", "mdp_integrate_group", "mdp_langevin_group",
    "mdp_md_set_image", "mdp_md_download_unwrapped", "mdp_msd_setup", "mdp_msd_sums", "mdp_msd_info", "mdp_msd_off",
    "mdp_rdf_setup", "mdp_rdf_counts", "mdp_rdf_info", "mdp_rdf_off",
    "mdp_adf_setup", "mdp_adf_counts", "mdp_adf_info", "mdp_adf_off",
    "mdp_coord_setup", "mdp_coord_read", "mdp_coord_info", "mdp_coord_off",
    "mdp_centro_setup", "mdp_centro_read", "mdp_centro_info", "mdp_centro_off",
    "mdp_cna_setup", "mdp_cna_read", "mdp_cna_counts", "mdp_cna_info", "mdp_cna_off",
    "mdp_profile_setup", "mdp_profile_range", "mdp_profile_exponent", "mdp_profile_sums", "mdp_profile_info", "mdp_profile_off",
    "mdp_rebomos_centre_paths", "mdp_rebomos_centre_blend_trips",
    "mdp_heatflux_sums", "mdp_md_download_vatom",
    "mdp_heat_setup", "mdp_heat_run", "mdp_heat_state", "mdp_heat_off",
    "mdp_indent_setup", "mdp_indent_run", "mdp_indent_state", "mdp_indent_off",
    "mdp_spring_setup", "mdp_spring_run", "mdp_spring_state", "mdp_spring_off",
    "mdp_gforce_setup", "mdp_gforce_run", "mdp_gforce_state", "mdp_gforce_off",
]


class MdpError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"libmdpair_hip: error {code}: {text}")
        self.code = code


_lib = None


def lib():
    """load the C-ABI library; no fallback of any kind if it is missing"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python __graft_entry__.py` (make -C lammps-plugins_amd)")
        try:
            # ONE HIP runtime per process: torch ships its own libamdhip64 under the same soname.  Whichever copy is
            # loaded first serves both; loaded after ours, torch finds "No HIP GPUs".  So torch goes first.
            import torch  # noqa: F401
        except ImportError:
            pass
        # (MDP_LIB_PATH: another build of the same library -- A/B runs of two kernel versions on one box)
        _lib = C.CDLL(os.environ.get("MDP_LIB_PATH") or LIB_PATH)
        _lib.mdp_last_error.restype = C.c_char_p
        _lib.mdp_md_ptr.restype = C.c_void_p
        _lib.mdp_device_bytes.restype = C.c_double
    return _lib


def profile_exponent(rng, natoms_total):
    """mdp_profile_exponent: the power of two a profile column with global range rng is scaled by -- the library's one copy of
    the rule (a pure host function: no context, no device)"""
    return int(lib().mdp_profile_exponent(C.c_double(float(rng)), C.c_longlong(int(natoms_total))))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def _slots(config, n):
    """the arguments of a set-up that takes n slots: their configurations and group bits (never of length 0)"""
    return (config * max(n, 1))(), (C.c_int * max(n, 1))()


def comm_library():
    """(name of the RCCL object the library binds, True when it is the test double of tests/native)"""
    buf = C.create_string_buffer(256)
    rc = lib().mdp_dd_comm_library(buf, C.c_int(256))
    if rc < 0:
        raise MdpError(rc, "no RCCL library could be loaded (MDP_RCCL_LIBRARY / librccl.so.1)")
    return buf.value.decode(), rc == 1


FAKE_RCCL = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "native",
                                          "libfake_rccl.so"))


def read_rebomos_file(path: str) -> RebomosParams:
    """product-side parser (csrc/potfile.cpp), mirrors PairREBOMoS::read_file"""
    p = RebomosParams()
    err = C.create_string_buffer(512)
    rc = lib().mdp_rebomos_read_file(path.encode(), C.byref(p), err, C.c_int(512))
    if rc:
        raise MdpError(rc, err.value.decode())
    return p


class AeamFile:
    """product-side AEAM potential file (csrc/potfile.cpp), mirrors PairAEAM::read_file + array2spline"""

    def __init__(self, path: str):
        self.h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = lib().mdp_aeam_file_read(path.encode(), C.byref(self.h), err, C.c_int(512))
        if rc:
            raise MdpError(rc, err.value.decode())
        ne, nn, na = C.c_int(), C.c_int(), C.c_int()
        mass = (C.c_double * 64)()
        names = C.create_string_buffer(64 * 16 + 16)
        lib().mdp_aeam_file_info(self.h, C.byref(ne), C.byref(nn), C.byref(na), mass, C.c_int(64), names,
                                 C.c_int(64 * 16 + 16))
        self.nelements, self.nnonangular, self.nangular = ne.value, nn.value, na.value
        self.mass = list(mass)[:ne.value]
        self.elements = names.value.decode().split()

    def build(self, ntypes: int | None = None, map_=None) -> AeamTables:
        ntypes = self.nelements if ntypes is None else ntypes
        m = np.ascontiguousarray([0] + list(range(ntypes)) if map_ is None else map_, dtype=np.int32)
        t = AeamTables()
        rc = lib().mdp_aeam_file_build(self.h, C.c_int(ntypes), _ip(m), C.byref(t))
        if rc:
            raise MdpError(rc, "mdp_aeam_file_build failed")
        return t

    def cut_table(self, t: AeamTables) -> np.ndarray:
        """(ntypes+1, ntypes+1) table of setfl->cut[i-1][j-1] (what init_one returns)"""
        ne = t.nelements
        cut = np.ctypeslib.as_array(t.cut, shape=(ne, ne))
        out = np.zeros((t.ntypes + 1, t.ntypes + 1))
        out[1:, 1:] = cut[:t.ntypes, :t.ntypes]
        return out

    def __del__(self):
        try:
            if self.h:
                lib().mdp_aeam_file_free(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


class _SerialLib:
    """the library behind one process-wide lock: used when several ranks run as threads of one process
    (resident.run_ranks); RCCL runs have one process per GPU and call the library directly"""
    import threading as _threading
    lock = _threading.RLock()

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        lock = self.lock

        def call(*a):
            with lock:
                return fn(*a)
        return call


class Context:
    """one mdp_ctx (one GPU sub-domain)"""
    serialize = False   # set by resident.run_ranks around threaded rehearsals

    def __init__(self, device: int = 0):
        self.L = _SerialLib(lib()) if Context.serialize else lib()
        self.h = C.c_void_p()
        rc = self.L.mdp_create(C.byref(self.h), C.c_int(device))
        if rc:
            raise MdpError(rc, "mdp_create failed (no usable HIP device?)")
        self._keep = []

    def close(self):
        if self.h:
            self.L.mdp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise MdpError(rc, self.L.mdp_last_error(self.h).decode())

    # ---------------- potentials
    def rebomos_set_params(self, params: RebomosParams):
        self._ck(self.L.mdp_rebomos_set_params(self.h, C.byref(params)))

    def aeam_set_tables(self, t: AeamTables):
        self._ck(self.L.mdp_aeam_set_tables(self.h, C.byref(t)))

    def set_stream(self, stream_ptr: int):
        self._ck(self.L.mdp_set_stream(self.h, C.c_void_p(stream_ptr)))

    def sync(self):
        self._ck(self.L.mdp_sync(self.h))

    def set_timing(self, on=True):
        self._ck(self.L.mdp_set_timing(self.h, C.c_int(1 if on else 0)))

    def get_timing(self):
        ms = (C.c_double * 8)()
        self._ck(self.L.mdp_get_timing(self.h, ms))
        return list(ms)

    # ---------------- host mode
    def set_atoms_host(self, nlocal, x_all, type_all, tag_all, ntypes, map_=None):
        x_all = np.ascontiguousarray(x_all, dtype=np.float64)
        type_all = np.ascontiguousarray(type_all, dtype=np.int32)
        tag_all = None if tag_all is None else np.ascontiguousarray(tag_all, dtype=np.int32)
        m = None if map_ is None else np.ascontiguousarray(map_, dtype=np.int32)
        self._ck(self.L.mdp_set_atoms_host(self.h, C.c_int(nlocal), C.c_int(len(x_all) - nlocal), _dp(x_all),
                                           _ip(type_all), _ip(tag_all), C.c_int(ntypes), _ip(m)))

    def set_positions_host(self, x_all):
        x_all = np.ascontiguousarray(x_all, dtype=np.float64)
        self._ck(self.L.mdp_set_positions_host(self.h, _dp(x_all)))

    def set_box_host(self, box):
        """Domain::h of the host's box (xprd, yprd, zprd, yz, xz, xy); None withdraws it"""
        if box is None:
            self._ck(self.L.mdp_set_box_host(self.h, None))
            return
        xy, xz, yz = box.tilt
        h = np.array([box.prd[0], box.prd[1], box.prd[2], yz, xz, xy], dtype=np.float64)
        self._ck(self.L.mdp_set_box_host(self.h, _dp(h)))

    def host_ghosts_derived(self):
        return bool(self.L.mdp_host_ghosts_derived(self.h))

    def set_neighbors_csr_host(self, numneigh, offset, neigh, skin):
        numneigh = np.ascontiguousarray(numneigh, dtype=np.int32)
        offset = np.ascontiguousarray(offset, dtype=np.int64)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        self._ck(self.L.mdp_set_neighbors_csr_host(self.h, C.c_int(len(numneigh)), _ip(numneigh),
                                                   offset.ctypes.data_as(C.POINTER(C.c_longlong)), _ip(neigh),
                                                   C.c_double(skin)))

    def set_skin(self, skin):
        self._ck(self.L.mdp_set_skin(self.h, C.c_double(skin)))

    def rebomos_host_list(self, on=True):
        self._ck(self.L.mdp_rebomos_host_list(self.h, C.c_int(1 if on else 0)))

    def aeam_device_lists(self, on=True):
        self._ck(self.L.mdp_aeam_device_lists(self.h, C.c_int(1 if on else 0)))

    def aeam_check_host_list(self, ilist, numneigh, rows, skin):
        ilist = np.ascontiguousarray(ilist, dtype=np.int32)
        numneigh = np.ascontiguousarray(numneigh, dtype=np.int32)
        ptrs = (C.POINTER(C.c_int) * len(rows))()
        for i, r in enumerate(rows):
            ptrs[i] = r.ctypes.data_as(C.POINTER(C.c_int))
        self._ck(self.L.mdp_aeam_check_host_list(self.h, C.c_int(len(ilist)), _ip(ilist), _ip(numneigh), ptrs,
                                                 C.c_double(skin)))

    def device_bytes(self) -> float:
        return float(self.L.mdp_device_bytes(self.h))

    def rebomos_check_host_list(self, ilist, numneigh, rows, cutneigh):
        """rows: list of int32 arrays, one per atom index (the LAMMPS firstneigh[] shape)"""
        ilist = np.ascontiguousarray(ilist, dtype=np.int32)
        numneigh = np.ascontiguousarray(numneigh, dtype=np.int32)
        ptrs = (C.POINTER(C.c_int) * len(rows))()
        for i, r in enumerate(rows):
            ptrs[i] = r.ctypes.data_as(C.POINTER(C.c_int))
        self._ck(self.L.mdp_rebomos_check_host_list(self.h, C.c_int(len(ilist)), _ip(ilist), _ip(numneigh), ptrs,
                                                    C.c_double(cutneigh)))

    def set_neighbors_paged_host(self, inum, gnum, ilist, numneigh, rows, skin):
        """rows: list of int32 arrays (one per atom index) -- exercises the LAMMPS int** path"""
        ilist = np.ascontiguousarray(ilist, dtype=np.int32)
        numneigh = np.ascontiguousarray(numneigh, dtype=np.int32)
        ptrs = (C.POINTER(C.c_int) * len(rows))()
        for i, r in enumerate(rows):
            ptrs[i] = r.ctypes.data_as(C.POINTER(C.c_int))
        self._ck(self.L.mdp_set_neighbors_host(self.h, C.c_int(inum), C.c_int(gnum), _ip(ilist), _ip(numneigh), ptrs,
                                               C.c_double(skin)))

    def rebomos_compute_host(self, nlocal, eflag=3, vflag=1):
        f = np.zeros((nlocal, 3))
        eng = C.c_double(0.0)
        vir = np.zeros(6)
        eatom = np.zeros(nlocal)
        vatom = np.zeros((nlocal, 6)) if vflag & 4 else None
        self._ck(self.L.mdp_rebomos_compute_host(self.h, C.c_int(eflag), C.c_int(vflag), _dp(f), C.byref(eng),
                                                 _dp(vir), _dp(eatom), _dp(vatom)))
        return dict(f=f, eng=eng.value, virial=vir, eatom=eatom, vatom=vatom)

    def aeam_density_host(self, nlocal, eflag=3, keep_fp=False):
        """keep_fp: fp (and rho) stay on the device (needs host_ghosts_derived())"""
        fp = None if keep_fp else np.zeros(nlocal)
        rho = None if keep_fp else np.zeros(nlocal)
        eng = C.c_double(0.0)
        eatom = np.zeros(nlocal)
        self._ck(self.L.mdp_aeam_density_host(self.h, C.c_int(eflag), _dp(fp), _dp(rho), C.byref(eng), _dp(eatom)))
        return dict(fp=fp, rho=rho, eng=eng.value, eatom=eatom)

    def aeam_force_host(self, nall, nlocal, fp_all, eflag=3, vflag=1):
        fp_all = None if fp_all is None else np.ascontiguousarray(fp_all, dtype=np.float64)
        f = np.zeros((nall, 3))
        eng = C.c_double(0.0)
        vir = np.zeros(6)
        eatom = np.zeros(nlocal)
        vatom = np.zeros((nall, 6)) if vflag & 4 else None
        self._ck(self.L.mdp_aeam_force_host(self.h, C.c_int(eflag), C.c_int(vflag), _dp(fp_all), _dp(f), C.byref(eng),
                                            _dp(vir), _dp(eatom), _dp(vatom)))
        return dict(f=f, eng=eng.value, virial=vir, eatom=eatom, vatom=vatom)

    # ---------------- resident mode
    def md_setup(self, cfg: MdConfig, x, v, type_, tag, mass, map_, ghost_owner, ghost_shift, ghost_type, ghost_tag):
        a = lambda arr, dt: np.ascontiguousarray(arr, dtype=dt)
        x, v, ghost_shift, mass = a(x, np.float64), a(v, np.float64), a(ghost_shift, np.float64), a(mass, np.float64)
        type_, tag, ghost_owner, ghost_type, ghost_tag = (a(type_, np.int32), a(tag, np.int32), a(ghost_owner, np.int32),
                                                          a(ghost_type, np.int32), a(ghost_tag, np.int32))
        m = None if map_ is None else a(map_, np.int32)
        self._ck(self.L.mdp_md_setup(self.h, C.byref(cfg), _dp(x), _dp(v), _ip(type_), _ip(tag), _dp(mass), _ip(m),
                                     _ip(ghost_owner), _dp(ghost_shift), _ip(ghost_type), _ip(ghost_tag)))

    def md_build_neighbors(self):
        self._ck(self.L.mdp_md_build_neighbors(self.h))

    def md_initial_integrate(self):
        self._ck(self.L.mdp_md_initial_integrate(self.h))

    def md_final_integrate(self):
        self._ck(self.L.mdp_md_final_integrate(self.h))

    def md_defer_final(self):
        self._ck(self.L.mdp_md_defer_final(self.h))

    def md_list_state(self):
        out = (C.c_double * 8)()
        self._ck(self.L.mdp_md_list_state(self.h, out))
        return dict(skin=out[0], inner_skin_cap=out[1], prune_buffer=out[2], late_builds=int(out[3]),
                    centre3_overflow=int(out[4]), centre3_list_mode=bool(out[5]))

    def md_final_initial_integrate(self):
        self._ck(self.L.mdp_md_final_initial_integrate(self.h))

    def md_compute(self, eflag=0, vflag=0):
        self._ck(self.L.mdp_md_compute(self.h, C.c_int(eflag), C.c_int(vflag)))

    def md_compute_begin(self, eflag=0, vflag=0):
        self._ck(self.L.mdp_md_compute_begin(self.h, C.c_int(eflag), C.c_int(vflag)))

    def md_compute_end(self, eflag=0, vflag=0):
        self._ck(self.L.mdp_md_compute_end(self.h, C.c_int(eflag), C.c_int(vflag)))

    def md_aeam_density(self, eflag=0):
        self._ck(self.L.mdp_md_aeam_density(self.h, C.c_int(eflag)))

    def md_aeam_force(self, eflag=0, vflag=0):
        self._ck(self.L.mdp_md_aeam_force(self.h, C.c_int(eflag), C.c_int(vflag)))

    def md_aeam_force_begin(self, eflag=0, vflag=0):
        self._ck(self.L.mdp_md_aeam_force_begin(self.h, C.c_int(eflag), C.c_int(vflag)))

    def md_aeam_state(self):
        """phases of the current aeam compute done so far, tiles that reach no remote ghost, tiles, whether ghost
        forces can be non-zero (see mdpair_hip.h)"""
        out = (C.c_int * 4)()
        self._ck(self.L.mdp_md_aeam_state(self.h, out))
        return dict(phase=int(out[0]), interior_tiles=int(out[1]), tiles=int(out[2]), ghost_forces=bool(out[3]))

    def md_thermo(self):
        out = (C.c_double * 9)()
        self._ck(self.L.mdp_md_thermo(self.h, out))
        o = list(out)
        return dict(ke=o[0], pe=o[1], virial=np.array(o[2:8]), maxdisp2=o[8])

    def md_download(self, nlocal, want=("x", "v", "f")):
        arrs = {k: (np.zeros((nlocal, 3)) if k in want else None) for k in ("x", "v", "f")}
        ea = np.zeros(nlocal) if "eatom" in want else None
        self._ck(self.L.mdp_md_download(self.h, _dp(arrs["x"]), _dp(arrs["v"]), _dp(arrs["f"]), _dp(ea)))
        arrs["eatom"] = ea
        return arrs

    def md_download_x_all(self, nall):
        x = np.zeros((max(nall, 1), 3))
        self._ck(self.L.mdp_md_download_x_all(self.h, _dp(x)))
        return x[:nall]

    def md_upload_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._ck(self.L.mdp_md_upload_x(self.h, _dp(x)))

    def md_ptr(self, name: str) -> int:
        p = self.L.mdp_md_ptr(self.h, name.encode())
        if not p:
            raise MdpError(-1, f"mdp_md_ptr({name}) returned NULL")
        return int(p)

    def rebomos_list_info(self):
        """shape of the style's Lennard-Jones lists after the last build (see mdpair_hip.h)"""
        out = (C.c_longlong * 8)()
        self._ck(self.L.mdp_rebomos_list_info(self.h, out))
        keys = ("tiled", "tiles", "union_stride", "union_max", "row_entries", "clusters", "large_tiles", "builds")
        return dict(zip(keys, (int(v) for v in out)))

    def rebomos_centre_paths(self, reset=True):
        """(waves of the lane-group centre kernels on the full-group path, waves on the general loops) over the computes
        run with MDP_CENTRE_COUNT=1 since the last reset (see mdpair_hip.h)"""
        out = (C.c_longlong * 2)()
        self._ck(self.L.mdp_rebomos_centre_paths(self.h, out, C.c_int(1 if reset else 0)))
        return int(out[0]), int(out[1])

    def rebomos_centre_blend_trips(self, reset=True):
        """trips of the first pair loop that took the G(cos) blend, over the waves on the full-group path of the computes
        run with MDP_CENTRE_COUNT=1 since its last reset (see mdpair_hip.h)"""
        out = C.c_longlong(0)
        self._ck(self.L.mdp_rebomos_centre_blend_trips(self.h, C.byref(out), C.c_int(1 if reset else 0)))
        return int(out.value)

    def md_neighbor_stats(self):
        out = (C.c_longlong * 8)()
        self._ck(self.L.mdp_md_neighbor_stats(self.h, out))
        return list(out)

    # ---------------- host mode with the integrator on the device (fix nve/mdp)
    def hnve_setup(self, dt, ftm2v, mass_per_type):
        m = np.ascontiguousarray(mass_per_type, dtype=np.float64)
        self._ck(self.L.mdp_hnve_setup(self.h, C.c_double(dt), C.c_double(ftm2v), _dp(m), C.c_int(len(m) - 1)))

    def hnve_off(self):
        self._ck(self.L.mdp_hnve_off(self.h))

    def hnve_upload_v(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        self._ck(self.L.mdp_hnve_upload_v(self.h, _dp(v)))

    def hnve_initial(self):
        m, d = C.c_int(0), C.c_int(0)
        self._ck(self.L.mdp_hnve_initial(self.h, C.byref(m), C.byref(d)))
        return bool(m.value), bool(d.value)

    def hnve_final(self):
        self._ck(self.L.mdp_hnve_final(self.h))

    def hnve_download(self, nlocal, want=("x", "v", "f")):
        out = {k: np.zeros((nlocal, 3)) for k in want}
        self._ck(self.L.mdp_hnve_download(self.h, _dp(out.get("x")), _dp(out.get("v")), _dp(out.get("f"))))
        return out

    # ---------------- Nose-Hoover chain thermostat of the integrate calls (fix nvt/mdp)
    def nhc_setup(self, t_start, t_stop, t_period, nf, tchain=3, tloop=1, drag=0.0, boltz=BOLTZ_METAL, mvv2e=1.0364269e-4):
        cfg = NhcConfig(t_start, t_stop, t_period, tchain, tloop, drag, nf, boltz, mvv2e)
        self._ck(self.L.mdp_nhc_setup(self.h, C.byref(cfg)))

    def nhc_run(self, first, last):
        self._ck(self.L.mdp_nhc_run(self.h, C.c_longlong(first), C.c_longlong(last)))

    def nhc_state(self):
        """{"temp", "target", "energy", "eta"[8], "eta_dot"[9], "eta_dotdot"[8], "raw"} of the last half-update"""
        out = np.zeros(NHC_STATE_LEN)
        self._ck(self.L.mdp_nhc_state(self.h, _dp(out)))
        return {"temp": out[0], "target": out[1], "energy": out[2], "eta": out[3:11].copy(), "eta_dot": out[11:20].copy(),
                "eta_dotdot": out[20:28].copy(), "raw": out}

    def nhc_set_state(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        assert raw.shape == (NHC_STATE_LEN,)
        self._ck(self.L.mdp_nhc_set_state(self.h, _dp(raw)))

    def nhc_off(self):
        self._ck(self.L.mdp_nhc_off(self.h))

    # ---------------- Langevin thermostat of the integrate calls (fix langevin/mdp)
    @staticmethod
    def _langevin_config(cfg, t_start, t_stop, t_period, seed, natoms, ratio=None, zero=False, tally=False,
                         boltz=BOLTZ_METAL, mvv2e=1.0364269e-4):
        cfg.t_start, cfg.t_stop, cfg.t_period, cfg.seed = t_start, t_stop, t_period, seed
        cfg.zero, cfg.tally, cfg.boltz, cfg.mvv2e, cfg.natoms = int(zero), int(tally), boltz, mvv2e, natoms
        for t in range(16):
            cfg.ratio[t] = 1.0
        for t, r in (ratio or {}).items():
            cfg.ratio[t] = r

    def langevin_setup(self, t_start, t_stop, t_period, seed, natoms, ratio=None, zero=False, tally=False,
                       boltz=BOLTZ_METAL, mvv2e=1.0364269e-4):
        """ratio: {type: ratio} of `scale` (1 for the other types)"""
        cfg = LangevinConfig()
        self._langevin_config(cfg, t_start, t_stop, t_period, seed, natoms, ratio, zero, tally, boltz, mvv2e)
        self._ck(self.L.mdp_langevin_setup(self.h, C.byref(cfg)))

    def langevin_baths(self, baths, boltz=BOLTZ_METAL, mvv2e=1.0364269e-4):
        """several thermostats on disjoint groups (mdp_langevin_baths): baths is a list of dicts with the keywords of
        langevin_setup (t_start, t_stop, t_period, seed, natoms, ratio, zero, tally) and `bit`, the bath's group bit"""
        n = len(baths)
        cfgs = (LangevinConfig * max(n, 1))()
        bits = (C.c_int * max(n, 1))()
        for k, b in enumerate(baths):
            b = dict(b)
            bits[k] = int(b.pop("bit"))
            self._langevin_config(cfgs[k], boltz=boltz, mvv2e=mvv2e, **b)
        self._ck(self.L.mdp_langevin_baths(self.h, C.c_int(n), cfgs, bits))

    def langevin_run(self, first, last):
        self._ck(self.L.mdp_langevin_run(self.h, C.c_longlong(first), C.c_longlong(last)))

    def langevin_tally(self, bath=None):
        """the thermostat energy (FixLangevin::compute_scalar; 0 without tally); with several baths their sum in bath
        order, or that of bath `bath`"""
        out = C.c_double(0.0)
        if bath is None:
            self._ck(self.L.mdp_langevin_tally(self.h, C.byref(out)))
        else:
            self._ck(self.L.mdp_langevin_tally_bath(self.h, C.c_int(int(bath)), C.byref(out)))
        return out.value

    def langevin_off(self):
        self._ck(self.L.mdp_langevin_off(self.h))

    # ---------------- constant-flux heat sources behind the final halves (fix heat/mdp)
    def heat_setup(self, sources, mvv2e=1.0364269e-4):
        """mdp_heat_setup: sources is a list of dicts eflux (energy / time, either sign), nevery, bit (the source's group bit)"""
        n = len(sources)
        cfgs, bits = _slots(HeatConfig, n)
        for k, s in enumerate(sources):
            cfgs[k].eflux, cfgs[k].nevery, cfgs[k].mvv2e = float(s["eflux"]), int(s["nevery"]), float(s.get("mvv2e", mvv2e))
            bits[k] = int(s["bit"])
        self._ck(self.L.mdp_heat_setup(self.h, C.c_int(n), cfgs, bits))

    def heat_run(self, first):
        self._ck(self.L.mdp_heat_run(self.h, C.c_longlong(first)))

    def heat_state(self, src):
        """source src after the last finished step (blocking): scale of its last application, vcm and the kinetic energy
        about the centre of mass before it (times ftm2v), M, applications so far, step of a latched error or -1"""
        out = np.zeros(HEAT_STATE_LEN)
        self._ck(self.L.mdp_heat_state(self.h, C.c_int(int(src)), _dp(out)))
        return dict(scale=float(out[0]), vcm=out[1:4].copy(), kecm=float(out[4]), mass=float(out[5]), applied=int(out[6]),
                    error_step=int(out[7]))

    def heat_off(self):
        self._ck(self.L.mdp_heat_off(self.h))

    # ---------------- indenters in front of the kicks (fix indent/mdp)
    def indent_setup(self, indenters):
        """mdp_indent_setup: indenters is a list of dicts shape ("sphere", "cylinder", "plane" or 0, 1, 2), k, r (a plane
        needs none), c (the centre at the run's first step, three numbers), and optionally dim (0, 1, 2: the cylinder's
        axis, the plane's normal), side ("out" / "in", "lo" / "hi" or 0 / 1), vel (three numbers), bit (the group bit; 0:
        every owned atom)"""
        n = len(indenters)
        cfgs, bits = _slots(IndentConfig, n)
        for k, q in enumerate(indenters):
            cfgs[k].shape = INDENT_SHAPES.get(q["shape"], q["shape"])
            cfgs[k].dim = int(q.get("dim", 0))
            cfgs[k].side = INDENT_SIDES.get(q.get("side", 0), q.get("side", 0))
            cfgs[k].k, cfgs[k].r = float(q["k"]), float(q.get("r", 0.0))
            cfgs[k].c[:] = [float(a) for a in q["c"]]
            cfgs[k].vel[:] = [float(a) for a in q.get("vel", (0.0, 0.0, 0.0))]
            bits[k] = int(q.get("bit", 0))
        self._ck(self.L.mdp_indent_setup(self.h, C.c_int(n), cfgs, bits))

    def indent_run(self, first):
        self._ck(self.L.mdp_indent_run(self.h, C.c_longlong(first)))

    def indent_state(self, k):
        """indenter k for the forces the context holds (blocking; runs their pass if no kick has yet): its energy, the
        force on it, the atoms in contact, the step these belong to, the centre at that step, passes since setup"""
        out = np.zeros(INDENT_STATE_LEN)
        self._ck(self.L.mdp_indent_state(self.h, C.c_int(int(k)), _dp(out)))
        return dict(energy=float(out[0]), force=out[1:4].copy(), contacts=int(out[4]), step=int(out[5]), centre=out[6:9].copy(),
                    passes=int(out[9]))

    def indent_off(self):
        self._ck(self.L.mdp_indent_off(self.h))

    # ---------------- tether springs in front of the kicks (fix spring/mdp)
    def spring_setup(self, springs):
        """mdp_spring_setup: springs is a list of dicts k, r0 (default 0), c (the tether point at the run's first step:
        three entries, None for a dimension that takes no part, LAMMPS' NULL), and optionally vel (three numbers), bit (the
        group bit; 0: every owned atom)"""
        n = len(springs)
        cfgs, bits = _slots(SpringConfig, n)
        for k, q in enumerate(springs):
            cfgs[k].k, cfgs[k].r0 = float(q["k"]), float(q.get("r0", 0.0))
            cfgs[k].c[:] = [0.0 if a is None else float(a) for a in q["c"]]
            cfgs[k].use[:] = [0 if a is None else 1 for a in q["c"]]
            cfgs[k].vel[:] = [float(a) for a in q.get("vel", (0.0, 0.0, 0.0))]
            bits[k] = int(q.get("bit", 0))
        self._ck(self.L.mdp_spring_setup(self.h, C.c_int(n), cfgs, bits))

    def spring_run(self, first):
        self._ck(self.L.mdp_spring_run(self.h, C.c_longlong(first)))

    def spring_state(self, k):
        """spring k for the forces the context holds (blocking; runs their pass if no kick has yet): its energy, ftotal
        (the force on the group, then sign(dr) |F|), the step these belong to, the unwrapped centre of mass, the tether
        point at that step, the group's mass and atoms, passes since setup"""
        out = np.zeros(SPRING_STATE_LEN)
        self._ck(self.L.mdp_spring_state(self.h, C.c_int(int(k)), _dp(out)))
        return dict(energy=float(out[0]), ftotal=out[1:5].copy(), step=int(out[5]), xcm=out[6:9].copy(), tether=out[9:12].copy(),
                    mass=float(out[12]), atoms=int(out[13]), passes=int(out[14]))

    def spring_off(self):
        self._ck(self.L.mdp_spring_off(self.h))

    # ---------------- prescribed group forces in front of the kicks (fix setforce/mdp, addforce/mdp, aveforce/mdp)
    def gforce_setup(self, slots):
        """mdp_gforce_setup: slots is a list of dicts kind ("set", "add", "ave" or 0, 1, 2), f (three entries, None for a
        dimension that is left alone, LAMMPS' NULL), and optionally bit (the group bit; 0: every owned atom).  They act in
        list order on an atom's force"""
        n = len(slots)
        cfgs, bits = _slots(GforceConfig, n)
        for k, q in enumerate(slots):
            cfgs[k].kind = GFORCE_KINDS.get(q["kind"], q["kind"])
            cfgs[k].f[:] = [0.0 if a is None else float(a) for a in q["f"]]
            cfgs[k].use[:] = [0 if a is None else 1 for a in q["f"]]
            bits[k] = int(q.get("bit", 0))
        self._ck(self.L.mdp_gforce_setup(self.h, C.c_int(n), cfgs, bits))

    def gforce_run(self, first):
        self._ck(self.L.mdp_gforce_run(self.h, C.c_longlong(first)))

    def gforce_state(self, k):
        """slot k for the forces the context holds (blocking; runs their pass if no kick has yet): its energy (addforce),
        the group's total force before the slot acted, the group's atoms, the step these belong to, the value written or
        added per dimension, passes since setup"""
        out = np.zeros(GFORCE_STATE_LEN)
        self._ck(self.L.mdp_gforce_state(self.h, C.c_int(int(k)), _dp(out)))
        return dict(energy=float(out[0]), ftotal=out[1:4].copy(), atoms=int(out[4]), step=int(out[5]), value=out[6:9].copy(),
                    passes=int(out[9]))

    def gforce_off(self):
        self._ck(self.L.mdp_gforce_off(self.h))

    # ---------------- FIRE minimiser of a resident one-brick context (minimize/mdp)
    def fire_setup(self, etol, ftol, maxiter, maxeval, **modify):
        """modify: the min_modify values of FIRE_DEFAULTS"""
        unknown = set(modify) - set(FIRE_DEFAULTS)
        if unknown:
            raise ValueError(f"fire_setup: unknown setting(s) {sorted(unknown)}")
        m = dict(FIRE_DEFAULTS, **modify)
        cfg = FireConfig(etol, ftol, int(maxiter), int(maxeval), m["dmax"], m["tmax"], m["tmin"], int(m["delaystep"]),
                         m["dtgrow"], m["dtshrink"], m["alpha0"], m["alphashrink"], int(bool(m["halfstepback"])),
                         int(bool(m["initialdelay"])))
        self._ck(self.L.mdp_fire_setup(self.h, C.byref(cfg)))

    def fire_iterate(self, n):
        """queues up to n iterations; the stop code the host has seen so far (0: running)"""
        stop = C.c_int(0)
        self._ck(self.L.mdp_fire_iterate(self.h, C.c_longlong(int(n)), C.byref(stop)))
        return stop.value

    def fire_state(self):
        """blocking: the minimiser's state (mdpair_hip.h, mdp_fire_state) as a dict"""
        out = np.zeros(FIRE_STATE_LEN)
        self._ck(self.L.mdp_fire_state(self.h, _dp(out)))
        keys = ("stop", "iterations", "evaluations", "dt", "alpha", "fnorm", "e_initial", "e_previous", "e_final",
                "reneighbors", "dtv", "dtv_prev", "s1", "s2", "mixed", "zeroed", "last_negative", "negatives", "vdotf",
                "fnorm_initial", "late")
        d = dict(zip(keys, (float(v) for v in out)))
        for k in ("stop", "iterations", "evaluations", "reneighbors", "mixed", "zeroed", "last_negative", "negatives", "late"):
            d[k] = int(d[k])
        d["criterion"] = FIRE_STOP[d["stop"]]
        return d

    def fire_off(self):
        self._ck(self.L.mdp_fire_off(self.h))

    def md_class_stats(self):
        """how the last compute's work was spread over the kernel classes (see mdpair_hip.h)"""
        out = (C.c_longlong * 32)()
        self._ck(self.L.mdp_md_class_stats(self.h, out))
        return [int(v) for v in out]

    def md_prune_stats(self):
        """dynamic pruning of the tile rows: prunings, late prunings, active, buffer (see mdpair_hip.h)"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_md_prune_stats(self.h, out))
        return dict(prunings=int(out[0]), late=int(out[1]), active=bool(out[2]), buffer=out[3] * 1e-6)

    # ---------------- domain decomposition on the device (csrc/domain.hip)
    def dd_setup(self, box, procgrid, rank, cutghost, self_remote=False, nonperiodic=(0, 0, 0)):
        """box: host.system.Box (restricted triclinic); procgrid: bricks per dimension; nonperiodic[d] = 1: no
        periodic images / no wrap in dimension d (LAMMPS boundary f / s)"""
        cfg = DdConfig()
        xy, xz, yz = (float(t) for t in box.tilt)
        for d in range(3):
            cfg.boxlo[d] = float(box.lo[d])
            cfg.procgrid[d] = int(procgrid[d])
        for k, val in enumerate((box.prd[0], box.prd[1], box.prd[2], yz, xz, xy)):
            cfg.h[k] = float(val)
        cfg.rank, cfg.cutghost, cfg.self_remote = int(rank), float(cutghost), 1 if self_remote else 0
        for d in range(3):
            cfg.nonperiodic[d] = 1 if nonperiodic[d] else 0
        self._ck(self.L.mdp_dd_setup(self.h, C.byref(cfg)))
        self._dd_nranks = int(procgrid[0]) * int(procgrid[1]) * int(procgrid[2])

    def dd_reneighbor(self):
        self._ck(self.L.mdp_dd_reneighbor(self.h))

    def dd_migrate_begin(self):
        cnt = (C.c_int * self._dd_nranks)()
        self._ck(self.L.mdp_dd_migrate_begin(self.h, cnt))
        return np.array(cnt, dtype=np.int64)

    def dd_migrate_pack(self, d_buf):
        self._ck(self.L.mdp_dd_migrate_pack(self.h, C.c_void_p(d_buf)))

    def dd_migrate_end(self, narrive, d_buf):
        self._ck(self.L.mdp_dd_migrate_end(self.h, C.c_int(int(narrive)), C.c_void_p(d_buf)))

    def dd_borders_begin(self):
        cnt = (C.c_int * self._dd_nranks)()
        self._ck(self.L.mdp_dd_borders_begin(self.h, cnt))
        return np.array(cnt, dtype=np.int64)

    def dd_borders_pack(self, d_buf):
        self._ck(self.L.mdp_dd_borders_pack(self.h, C.c_void_p(d_buf)))

    def dd_borders_end(self, recv_counts, d_buf):
        rc = (C.c_int * self._dd_nranks)(*[int(v) for v in recv_counts])
        self._ck(self.L.mdp_dd_borders_end(self.h, rc, C.c_void_p(d_buf)))

    def dd_info(self):
        out = (C.c_longlong * 8)()
        sc, rc = (C.c_int * self._dd_nranks)(), (C.c_int * self._dd_nranks)()
        self._ck(self.L.mdp_dd_info(self.h, out, sc, rc))
        keys = ("nlocal", "nself", "nsend", "nrecv", "reneighbors", "left_last", "nranks", "rank")
        d = dict(zip(keys, (int(v) for v in out)))
        d["send_counts"], d["recv_counts"] = np.array(sc, dtype=np.int64), np.array(rc, dtype=np.int64)
        return d

    def dd_forward_pack(self, d_buf):
        self._ck(self.L.mdp_dd_forward_pack(self.h, C.c_void_p(d_buf)))

    def dd_forward_unpack(self, d_buf):
        self._ck(self.L.mdp_dd_forward_unpack(self.h, C.c_void_p(d_buf)))

    def dd_forward_scalar_pack(self, d_buf):
        self._ck(self.L.mdp_dd_forward_scalar_pack(self.h, C.c_void_p(d_buf)))

    def dd_forward_scalar_unpack(self, d_buf):
        self._ck(self.L.mdp_dd_forward_scalar_unpack(self.h, C.c_void_p(d_buf)))

    def dd_reverse_pack(self, d_buf):
        self._ck(self.L.mdp_dd_reverse_pack(self.h, C.c_void_p(d_buf)))

    def dd_reverse_unpack(self, d_buf):
        self._ck(self.L.mdp_dd_reverse_unpack(self.h, C.c_void_p(d_buf)))

    # ---------------- RCCL transport inside the library (csrc/comm_rccl.hip)
    def dd_comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self.L.mdp_dd_comm_unique_id(buf)
        if rc:
            raise MdpError(rc, "mdp_dd_comm_unique_id failed (RCCL not loadable?)")
        return buf.raw

    def dd_comm_init(self, id128: bytes):
        self._ck(self.L.mdp_dd_comm_init(self.h, C.c_char_p(id128)))

    def dd_comm_reneighbor(self):
        self._ck(self.L.mdp_dd_comm_reneighbor(self.h))

    def dd_comm_forward_begin(self):
        self._ck(self.L.mdp_dd_comm_forward_begin(self.h))

    def dd_comm_forward_end(self):
        self._ck(self.L.mdp_dd_comm_forward_end(self.h))

    def dd_comm_forward_scalar(self):
        self._ck(self.L.mdp_dd_comm_forward_scalar(self.h))

    def dd_comm_reverse(self):
        self._ck(self.L.mdp_dd_comm_reverse(self.h))

    def dd_comm_aeam_exchange_begin(self, with_reverse=True):
        self._ck(self.L.mdp_dd_comm_aeam_exchange_begin(self.h, C.c_int(1 if with_reverse else 0)))

    def dd_comm_aeam_exchange_end(self):
        self._ck(self.L.mdp_dd_comm_aeam_exchange_end(self.h))

    def dd_comm_step_begin(self, with_final=False, force_rebuild=-1, eflag=0, vflag=0):
        r = C.c_int(0)
        self._ck(self.L.mdp_dd_comm_step_begin(self.h, C.c_int(1 if with_final else 0), C.c_int(force_rebuild), C.c_int(eflag),
                                               C.c_int(vflag), C.byref(r)))
        return bool(r.value)

    def dd_comm_step_end(self, eflag=0, vflag=0, defer_final=False):
        self._ck(self.L.mdp_dd_comm_step_end(self.h, C.c_int(eflag), C.c_int(vflag), C.c_int(1 if defer_final else 0)))

    def dd_comm_step_info(self):
        out = (C.c_longlong * 8)()
        self._ck(self.L.mdp_dd_comm_step_info(self.h, out))
        names = {-1: "undecided (trial running)", 0: "split", 1: "lead", 2: "blocking", 3: "first", 4: "inline"}
        return dict(aeam_phased=int(out[0]), ghost_forces=bool(out[1]), reneighbored=bool(out[2]), reneighbors=int(out[3]),
                    dangerous=int(out[4]), overlap_policy=names.get(int(out[5]), str(int(out[5]))),
                    overlap_policy_fixed_by_env=bool(out[6]), overlap_policy_trial_ms=int(out[7]) * 1.0e-6)

    def dd_comm_allreduce(self, values, op=0):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._ck(self.L.mdp_dd_comm_allreduce(self.h, _dp(v), C.c_int(len(v)), C.c_int(op)))
        return v

    def md_moved_async(self):
        """(moved, dangerous) of the check launched by the previous call; launches the next one"""
        m, d = C.c_int(0), C.c_int(0)
        self._ck(self.L.mdp_md_moved_async(self.h, C.byref(m), C.byref(d)))
        return bool(m.value), bool(d.value)

    def md_integrate_check(self, with_final=False):
        """initial_integrate (after the pending final half-kick if with_final) + md_moved_async in one kernel"""
        m, d = C.c_int(0), C.c_int(0)
        self._ck(self.L.mdp_md_integrate_check(self.h, C.c_int(1 if with_final else 0), C.byref(m), C.byref(d)))
        return bool(m.value), bool(d.value)

    def md_download_int(self, name: str, nlocal: int):
        out = np.zeros(max(nlocal, 1), dtype=np.int32)
        self._ck(self.L.mdp_md_download_int(self.h, name.encode(), _ip(out)))
        return out[:nlocal]

    # ---------------- groups: the owned atoms' mask and the bits the integrate calls honour
    def _mask_ptr(self, mask):
        if mask is None:
            return None, None
        m = np.ascontiguousarray(mask, dtype=np.int32)
        keep = m if len(m) else np.zeros(1, dtype=np.int32)   # (an empty brick still SETS a mask: NULL withdraws it)
        return keep, _ip(keep)

    def md_set_mask(self, mask):
        """resident mode: atom->mask of the owned atoms in the current device order (md_download_int("tag") gives it);
        None withdraws the mask"""
        keep, ptr = self._mask_ptr(mask)
        self._ck(self.L.mdp_md_set_mask(self.h, ptr))

    def hnve_set_mask(self, mask):
        """host-linked mode: atom->mask of the owned atoms in the host's order, after every set_atoms_host; None withdraws it"""
        keep, ptr = self._mask_ptr(mask)
        self._ck(self.L.mdp_hnve_set_mask(self.h, ptr))

    def integrate_group(self, groupbit):
        """the integrate calls advance the atoms with mask & groupbit only (0: every atom)"""
        self._ck(self.L.mdp_integrate_group(self.h, C.c_int(int(groupbit))))

    def langevin_group(self, groupbit):
        """the Langevin force goes to the atoms with mask & groupbit (inside the integrate group) only (0: every atom)"""
        self._ck(self.L.mdp_langevin_group(self.h, C.c_int(int(groupbit))))

    # ---------------- image flags, unwrapped positions and the mean-squared displacement (csrc/msd.hip)
    def md_set_image(self, image):
        """resident mode: atom->image (LAMMPS' 32-bit imageint) of the owned atoms in the current device order, as
        md_set_mask takes the mask; None withdraws it.  md_download_int("image") reads it back."""
        keep, ptr = self._mask_ptr(image)
        self._ck(self.L.mdp_md_set_image(self.h, ptr))

    def md_download_unwrapped(self, nlocal):
        """x + h . image of the owned atoms in device order"""
        xu = np.zeros((max(nlocal, 1), 3))
        self._ck(self.L.mdp_md_download_unwrapped(self.h, _dp(xu)))
        return xu[:nlocal]

    def msd_setup(self, ntag, x0_by_tag=None, groupbit=0):
        """starts a measurement: x0_by_tag[ntag][3] the unwrapped origins of ALL atoms, [tag - 1]; None: the owned atoms'
        current unwrapped positions (one rank only).  groupbit 0: every atom"""
        x0 = None if x0_by_tag is None else np.ascontiguousarray(x0_by_tag, dtype=np.float64)
        if x0 is not None and x0.shape != (int(ntag), 3):
            raise ValueError(f"msd_setup: x0_by_tag must be [{int(ntag)}][3], not {x0.shape}")
        self._ck(self.L.mdp_msd_setup(self.h, C.c_int(int(ntag)), _dp(x0), C.c_int(int(groupbit))))

    def msd_sums(self, shift=None):
        """this rank's sums over the group: [sum dx^2, dy^2, dz^2, count, sum m xu (3), sum m], d = xu - x0 - shift"""
        sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        out = np.zeros(8)
        self._ck(self.L.mdp_msd_sums(self.h, _dp(sh), _dp(out)))
        return out

    def msd_info(self):
        """whether a measurement is on, its ntag and group bit, and its serial (unique in the process per msd_setup)"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_msd_info(self.h, out))
        return dict(on=bool(out[0]), ntag=int(out[1]), groupbit=int(out[2]), serial=int(out[3]))

    def msd_off(self):
        self._ck(self.L.mdp_msd_off(self.h))

    # ---------------- pair-distance histograms: g(r) and coordination numbers (csrc/rdf.hip)
    def rdf_setup(self, nbin, cutoff, pairs, member_by_tag=None):
        """starts a measurement: pairs = [(ilo, ihi, jlo, jhi), ...] inclusive ranges of LAMMPS types, one column each;
        member_by_tag[t - 1] non-zero: the atom with tag t belongs to the group (ALL atoms of the system); None: every atom"""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 4)
        cols = [np.ascontiguousarray(pr[:, k]) for k in range(4)]
        mem = None if member_by_tag is None else np.ascontiguousarray(np.asarray(member_by_tag) != 0, dtype=np.uint8)
        self._ck(self.L.mdp_rdf_setup(self.h, C.c_int(int(nbin)), C.c_double(float(cutoff)), C.c_int(len(pr)), _ip(cols[0]),
                                      _ip(cols[1]), _ip(cols[2]), _ip(cols[3]), C.c_int(0 if mem is None else len(mem)),
                                      None if mem is None else mem.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def rdf_counts(self):
        """this rank's (hist[npair][nbin], icount, jcount, dup) as int64"""
        info = self.rdf_info()
        nbin, npair = max(info["nbin"], 1), max(info["npair"], 1)
        hist = np.zeros((npair, nbin), dtype=np.int64)
        cnt = np.zeros((3, npair), dtype=np.int64)
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
        self._ck(self.L.mdp_rdf_counts(self.h, lp(hist), lp(cnt[0]), lp(cnt[1]), lp(cnt[2])))
        return hist, cnt[0].copy(), cnt[1].copy(), cnt[2].copy()

    def rdf_info(self):
        """whether a measurement is on, its nbin and npair, and its serial (unique in the process per rdf_setup)"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_rdf_info(self.h, out))
        return dict(on=bool(out[0]), nbin=int(out[1]), npair=int(out[2]), serial=int(out[3]))

    def rdf_off(self):
        self._ck(self.L.mdp_rdf_off(self.h))

    # ---------------- bond-angle histograms: the angular distribution function (csrc/adf.hip)
    def adf_setup(self, nbin, ordinate, triples, member_by_tag=None):
        """starts a measurement: triples = [(ilo, ihi, jlo, jhi, klo, khi, rjin, rjout, rkin, rkout), ...] with inclusive ranges
        of LAMMPS types and the two shells, one pair of columns each; ordinate ADF_DEGREE / _RADIAN / _COSINE or its name;
        member_by_tag as in rdf_setup"""
        tr = np.ascontiguousarray(triples, dtype=np.float64).reshape(-1, 10)
        ty = [np.ascontiguousarray(tr[:, k], dtype=np.int32) for k in range(6)]
        rr = [np.ascontiguousarray(tr[:, k]) for k in range(6, 10)]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        mem = None if member_by_tag is None else np.ascontiguousarray(np.asarray(member_by_tag) != 0, dtype=np.uint8)
        self._ck(self.L.mdp_adf_setup(self.h, C.c_int(int(nbin)), C.c_int(int(ADF_ORDINATES.get(ordinate, ordinate))), C.c_int(len(tr)),
                                      *[_ip(a) for a in ty], *[dp(a) for a in rr], C.c_int(0 if mem is None else len(mem)),
                                      None if mem is None else mem.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def adf_counts(self):
        """this rank's (hist[ntriple][nbin], icount[ntriple]) as int64"""
        info = self.adf_info()
        hist = np.zeros((max(info["ntriple"], 1), max(info["nbin"], 1)), dtype=np.int64)
        icount = np.zeros(len(hist), dtype=np.int64)
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
        self._ck(self.L.mdp_adf_counts(self.h, lp(hist), lp(icount)))
        return hist, icount

    def adf_info(self):
        """whether a measurement is on, its nbin and ntriple, and its serial (unique in the process per adf_setup)"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_adf_info(self.h, out))
        return dict(on=bool(out[0]), nbin=int(out[1]), ntriple=int(out[2]), serial=int(out[3]))

    def adf_off(self):
        self._ck(self.L.mdp_adf_off(self.h))

    # ---------------- per-atom structure: coordination numbers and the centro-symmetry parameter (csrc/coord.hip, centro.hip)
    def coord_setup(self, cutoff, ranges, group_bit=0):
        """starts a measurement: ranges = [(jlo, jhi), ...] inclusive ranges of LAMMPS types, one column each; group_bit 0: every
        owned atom is a centre, else the atoms whose mask has the bit (partners of any group count)"""
        rg = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
        lo, hi = np.ascontiguousarray(rg[:, 0]), np.ascontiguousarray(rg[:, 1])
        self._ck(self.L.mdp_coord_setup(self.h, C.c_double(float(cutoff)), C.c_int(len(rg)), _ip(lo), _ip(hi), C.c_int(int(group_bit))))

    def coord_read(self, nlocal):
        """this rank's (tags[nlocal], values[nlocal][ncol]) in the owned order of md_download; 0 outside the group"""
        ncol = max(self.coord_info()["ncol"], 1)
        tags = np.zeros(max(nlocal, 1), dtype=np.int32)
        vals = np.zeros((max(nlocal, 1), ncol))
        self._ck(self.L.mdp_coord_read(self.h, _ip(tags), _dp(vals)))
        return tags[:nlocal], vals[:nlocal]

    def coord_info(self):
        """whether a measurement is on, its columns and group bit, and its serial (unique in the process per coord_setup)"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_coord_info(self.h, out))
        return dict(on=bool(out[0]), ncol=int(out[1]), groupbit=int(out[2]), serial=int(out[3]))

    def coord_off(self):
        self._ck(self.L.mdp_coord_off(self.h))

    def centro_setup(self, nnn, cutoff=None, group_bit=0):
        """starts a measurement over the nnn nearest neighbours (even; "fcc" = 12, "bcc" = 8) inside cutoff (None: the ghost
        shell's limit, cutghost - skin); group_bit as in coord_setup"""
        n = CENTRO_LATTICE.get(nnn, nnn)
        self._ck(self.L.mdp_centro_setup(self.h, C.c_int(int(n)), C.c_double(0.0 if cutoff is None else float(cutoff)),
                                         C.c_int(int(group_bit))))

    def centro_read(self, nlocal):
        """this rank's (tags[nlocal], values[nlocal]) in the owned order of md_download; 0 outside the group and for a centre with
        fewer than nnn atoms inside the cutoff (centro_info()["few"] counts those)"""
        tags = np.zeros(max(nlocal, 1), dtype=np.int32)
        vals = np.zeros(max(nlocal, 1))
        self._ck(self.L.mdp_centro_read(self.h, _ip(tags), _dp(vals)))
        return tags[:nlocal], vals[:nlocal]

    def centro_info(self):
        """whether a measurement is on, its nnn, the centres with fewer than nnn partners at the last read, and its serial"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_centro_info(self.h, out))
        return dict(on=bool(out[0]), nnn=int(out[1]), few=int(out[2]), serial=int(out[3]))

    def centro_off(self):
        self._ck(self.L.mdp_centro_off(self.h))

    # ---------------- per-atom structure: the common neighbour analysis (csrc/cna.hip)
    def cna_setup(self, cutoff, group_bit=0):
        """starts a measurement over the neighbours inside cutoff (0.8536 a for fcc and hcp, 1.207 a for bcc); group_bit as in
        coord_setup"""
        self._ck(self.L.mdp_cna_setup(self.h, C.c_double(float(cutoff)), C.c_int(int(group_bit))))

    def cna_read(self, nlocal):
        """this rank's (tags[nlocal], values[nlocal]) in the owned order of md_download: 1 fcc, 2 hcp, 3 bcc, 4 icosahedral,
        5 other, 0 outside the group"""
        tags = np.zeros(max(nlocal, 1), dtype=np.int32)
        vals = np.zeros(max(nlocal, 1))
        self._ck(self.L.mdp_cna_read(self.h, _ip(tags), _dp(vals)))
        return tags[:nlocal], vals[:nlocal]

    def cna_counts(self):
        """int64[6]: this rank's group atoms with pattern 0 .. 5 at the last read, counted on the device"""
        out = (C.c_longlong * 6)()
        self._ck(self.L.mdp_cna_counts(self.h, out))
        return np.array(list(out), dtype=np.int64)

    def cna_info(self):
        """whether a measurement is on, the centres with more than CNA_MAXNEAR neighbours at the last read, and its serial"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_cna_info(self.h, out))
        return dict(on=bool(out[0]), over=int(out[2]), serial=int(out[3]))

    def cna_off(self):
        self._ck(self.L.mdp_cna_off(self.h))

    # ---------------- binned mass, momentum and kinetic energy (csrc/profile.hip)
    def profile_setup(self, dims, nbins, group_bit=0):
        """starts a measurement: bins over the box in the distinct dimensions dims (0, 1, 2; the first slowest) with nbins[k]
        bins each; group_bit 0: every owned atom, else the atoms whose mask has the bit"""
        dm = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        nb = np.ascontiguousarray(nbins, dtype=np.int32).reshape(-1)
        if len(dm) != len(nb):
            raise ValueError("profile_setup: one number of bins per dimension")
        self._ck(self.L.mdp_profile_setup(self.h, C.c_int(len(dm)), _ip(dm), _ip(nb), C.c_int(int(group_bit))))

    def profile_range(self):
        """this rank's max |t_k| of the terms (m, m vx, m vy, m vz, m v.v) over the group's owned atoms"""
        out = (C.c_double * PROFILE_W)()
        self._ck(self.L.mdp_profile_range(self.h, out))
        return np.array(out[:], dtype=np.float64)

    def profile_exponent(self, rng, natoms_total):
        """the power of two a column with global range rng is scaled by (the library's one copy of the rule)"""
        return profile_exponent(rng, natoms_total)

    def profile_sums(self, exponents):
        """this rank's (count[rows], sums[rows][5]) as int64, the terms scaled by 2^exponents[k] and rounded"""
        rows = max(self.profile_info()["rows"], 1)
        ex = (C.c_int * PROFILE_W)(*[int(e) for e in exponents])
        count = np.zeros(rows, dtype=np.int64)
        sums = np.zeros((rows, PROFILE_W), dtype=np.int64)
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
        self._ck(self.L.mdp_profile_sums(self.h, ex, lp(count), lp(sums)))
        return count, sums

    def profile_info(self):
        """whether a measurement is on, its rows and dimensions, and its serial (unique in the process per profile_setup)"""
        out = (C.c_longlong * 4)()
        self._ck(self.L.mdp_profile_info(self.h, out))
        return dict(on=bool(out[0]), rows=int(out[1]), ndim=int(out[2]), serial=int(out[3]))

    def profile_off(self):
        self._ck(self.L.mdp_profile_off(self.h))

    # ---------------- the heat current from the per-atom tallies of the last compute (csrc/heatflux.hip)
    def heatflux_sums(self, group_bit=0):
        """this rank's sums over the group's owned atoms: [sum (ke + pe) v (3), sum W.v (3), count, sum (ke + pe)]; needs the last
        compute to have run with eflag | 2 and vflag | 4"""
        out = np.zeros(8)
        self._ck(self.L.mdp_heatflux_sums(self.h, C.c_int(int(group_bit)), _dp(out)))
        return out

    def md_download_vatom(self, nlocal):
        """the owned atoms' per-atom virial [nlocal][6] (xx yy zz xy xz yz) in device order, under the rule of heatflux_sums"""
        va = np.zeros((nlocal, 6))
        self._ck(self.L.mdp_md_download_vatom(self.h, _dp(va)))
        return va

    # halo plumbing (device pointers as ints)
    def md_pack_x(self, n, d_sendlist, d_shift, d_buf):
        self._ck(self.L.mdp_md_pack_x(self.h, C.c_int(n), C.c_void_p(d_sendlist), C.c_void_p(d_shift), C.c_void_p(d_buf)))

    def md_unpack_x(self, first_ghost, n, d_buf):
        self._ck(self.L.mdp_md_unpack_x(self.h, C.c_int(first_ghost), C.c_int(n), C.c_void_p(d_buf)))

    def md_pack_scalar(self, which, n, d_sendlist, d_buf):
        self._ck(self.L.mdp_md_pack_scalar(self.h, C.c_int(which), C.c_int(n), C.c_void_p(d_sendlist), C.c_void_p(d_buf)))

    def md_unpack_scalar(self, which, first_ghost, n, d_buf):
        self._ck(self.L.mdp_md_unpack_scalar(self.h, C.c_int(which), C.c_int(first_ghost), C.c_int(n), C.c_void_p(d_buf)))

    def md_pack_ghost_f(self, first_ghost, n, d_buf):
        self._ck(self.L.mdp_md_pack_ghost_f(self.h, C.c_int(first_ghost), C.c_int(n), C.c_void_p(d_buf)))

    def md_unpack_add_f(self, n, d_sendlist, d_buf):
        self._ck(self.L.mdp_md_unpack_add_f(self.h, C.c_int(n), C.c_void_p(d_sendlist), C.c_void_p(d_buf)))

    def md_fold_self_ghost_f(self):
        self._ck(self.L.mdp_md_fold_self_ghost_f(self.h))
