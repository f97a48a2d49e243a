"""Resident-mode MD driver (host side): one brick of the box per GPU, set up once, then stepped entirely on the GPU
through the C-ABI.  This is the small slice of the LAMMPS host around Pair::compute() that the bench and the tests
need (Verlet::run loop of fix nve, thermo, `neigh_modify every 1 check yes`, the transport of the bricks' exchanges);
the arithmetic and the domain decomposition all happen in libmdpair_hip.so.  (The round-1 host-planned decomposition,
kept as the independent reference of the tests, lives in tests/hostplan.py.)"""
from __future__ import annotations

import ctypes as C
import os as _os

import numpy as np

from . import capi
from . import system as S



# ---------------------------------------------------------------------------------------------------
# Device-side domain decomposition (csrc/domain.hip): every rank keeps ONE brick, remaps / migrates /
# re-derives its ghosts on the GPU at each reneighboring and only exchanges counts and packed records.
# ---------------------------------------------------------------------------------------------------

IMAGE0 = 512 | 512 << 10 | 512 << 20   # LAMMPS' imageint of the central image: (ix + 512) | (iy + 512) << 10 | (iz + 512) << 20


def image_counts(image):
    """imageint [n] -> the counts (ix, iy, iz) [n][3]"""
    im = np.asarray(image, dtype=np.int64)
    return np.stack([(im & 1023) - 512, ((im >> 10) & 1023) - 512, ((im >> 20) & 1023) - 512], axis=1)


def image_pack(counts):
    """the counts (ix, iy, iz) [n][3] -> imageint [n]; a field wraps modulo 1024"""
    c = np.asarray(counts, dtype=np.int64) + 512
    return ((c[:, 0] & 1023) | (c[:, 1] & 1023) << 10 | (c[:, 2] & 1023) << 20).astype(np.int32)


class Transport:
    """all-to-all of device buffers between the ranks of a torch.distributed group.  backend "nccl" is
    RCCL over xGMI (device buffers go straight in); any other backend is a rehearsal path for boxes with
    fewer GPUs than ranks: buffers are staged through the host around each collective."""

    def __init__(self, dist_module, device, stage_host: bool):
        import torch
        self.torch, self.dist, self.device, self.stage_host = torch, dist_module, device, stage_host
        self.on_gpu = torch.device(device).type == "cuda"
        self.world = dist_module.get_world_size()
        self.rank = dist_module.get_rank()

    def counts(self, send_counts: np.ndarray) -> np.ndarray:
        """recv[q] = what rank q sends to me.  Every rank gathers the whole count matrix (world^2 integers), so it
        also knows whether ANY rank has something to send: an exchange that is empty everywhere is skipped by all
        ranks alike (no collective is ever issued with empty tensors on every rank)."""
        torch = self.torch
        dev = "cpu" if self.stage_host else self.device
        s = torch.as_tensor(np.asarray(send_counts, dtype=np.int64), device=dev)
        rows = [torch.empty_like(s) for _ in range(self.world)]
        self.dist.all_gather(rows, s)
        m = torch.stack(rows).cpu().numpy()          # m[q][r]: rank q -> rank r
        self.last_total = int(m.sum())
        return m[:, self.rank].copy()

    def exchange(self, send, send_counts, recv_counts, width: int, recv=None, async_op=False):
        """send: flat float64 device tensor of sum(send_counts)*width; returns (recv tensor, work or None)"""
        torch = self.torch
        nrecv = int(np.sum(recv_counts)) * width
        if recv is None:
            recv = torch.empty(max(nrecv, 1), dtype=torch.float64, device=self.device)
        ins = [int(c) * width for c in send_counts]
        outs = [int(c) * width for c in recv_counts]
        nsend = sum(ins)
        if getattr(self, "last_total", 1) == 0 and nsend == 0 and nrecv == 0:
            return recv, None                    # nothing travels anywhere (decided from the gathered count matrix)
        if not self.stage_host:
            w = self.dist.all_to_all_single(recv[:nrecv], send[:nsend], outs, ins, async_op=async_op)
            return recv, w
        if self.on_gpu:
            torch.cuda.synchronize()
        o, i = recv[:nrecv].cpu(), send[:nsend].cpu()
        self.dist.all_to_all_single(o, i, outs, ins)
        recv[:nrecv].copy_(o)
        if self.on_gpu:
            torch.cuda.synchronize()
        return recv, None

    def any(self, flag: bool) -> bool:
        torch = self.torch
        t = torch.tensor([1.0 if flag else 0.0], device="cpu" if self.stage_host else self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return bool(t.item() > 0)

    def sum(self, values):
        torch = self.torch
        t = torch.tensor(list(values), dtype=torch.float64, device="cpu" if self.stage_host else self.device)
        self.dist.all_reduce(t)
        return t.cpu().numpy()


class NativeTransport:
    """The exchanges done INSIDE the library on RCCL (csrc/comm_rccl.hip: grouped ncclSend/ncclRecv between the
    bricks' GPUs) -- what a C++ host uses.  Python only bootstraps the communicator: rank 0 creates the 128-byte
    id, `bcast` hands it to every rank (torch.distributed broadcast, MPI_Bcast, ...)."""
    native = True
    stage_host = False

    def __init__(self, world: int, rank: int, bcast=None):
        self.world, self.rank = world, rank
        self.bcast = bcast if bcast is not None else (lambda b: b)
        self.ctx = None

    def attach(self, ctx: capi.Context):
        uid = ctx.dd_comm_unique_id() if self.rank == 0 else bytes(128)
        ctx.dd_comm_init(self.bcast(uid))
        self.ctx = ctx

    def any(self, flag: bool) -> bool:
        return bool(self.ctx.dd_comm_allreduce([1.0 if flag else 0.0], op=1)[0] > 0)

    def sum(self, values):
        return self.ctx.dd_comm_allreduce(list(values), op=0)


def rdf_normalise(hist, icount, jcount, dup, cutoff, volume):
    """LAMMPS' compute rdf array [nbin][1 + 2 npair] from rank-summed counts (DeviceDomain.rdf_read): column 0 the bin centres,
    then g(r) and the coordination number per pair.  volume = xprd yprd zprd, triclinic included."""
    hist = np.atleast_2d(np.asarray(hist, dtype=np.float64))
    npair, nbin = hist.shape
    delr = cutoff / nbin
    const = 4.0 * np.pi / (3.0 * volume)
    b = np.arange(nbin, dtype=np.float64)
    vfrac = const * (((b + 1.0) * delr) ** 3 - (b * delr) ** 3)
    out = np.zeros((nbin, 1 + 2 * npair))
    out[:, 0] = (b + 0.5) * delr
    for m in range(npair):
        ic, jc, du = float(icount[m]), float(jcount[m]), float(dup[m])
        normfac = jc - du / ic if ic > 0 else 0.0
        den = vfrac * normfac * ic
        g = np.divide(hist[m], den, out=np.zeros(nbin), where=den != 0.0)
        out[:, 1 + 2 * m] = g
        out[:, 2 + 2 * m] = np.cumsum(g * vfrac * normfac)
    return out


ADF_RANGE = dict(degree=(0.0, 180.0), radian=(0.0, np.pi), cosine=(-1.0, 1.0))


def adf_normalise(hist, icount, nbin, ordinate="degree", cumulative="fraction"):
    """compute adf/mdp's array [nbin][1 + 2 ntriple] from rank-summed counts (DeviceDomain.adf_read): column 0 the bin
    centres of the ordinate, then per triple hist / (count delta) with count = sum(hist) (it integrates to 1; 0 without a
    count) and the running sum of hist over count (cumulative fraction) or over icount (cumulative centre: angles per
    central atom)."""
    hist = np.atleast_2d(np.asarray(hist, dtype=np.float64))
    lo, hi = ADF_RANGE[ordinate]
    delta = (hi - lo) / nbin
    out = np.zeros((nbin, 1 + 2 * len(hist)))
    out[:, 0] = lo + (np.arange(nbin) + 0.5) * delta
    for m, h in enumerate(hist):
        count = h.sum()
        den = count if cumulative == "fraction" else float(icount[m])
        if cumulative not in ("fraction", "centre"):
            raise ValueError(f"adf_normalise: cumulative {cumulative!r}")
        out[:, 1 + 2 * m] = h / (count * delta) if count > 0 else 0.0
        out[:, 2 + 2 * m] = np.cumsum(h) / den if den > 0 else 0.0
    return out


def profile_split(q):
    """an int64 array as two float64 arrays (q >> 31, q & (2^31 - 1)): both halves, and their sums over up to 2^22 ranks, are
    whole numbers below 2^53, so a transport that adds doubles adds them exactly"""
    q = np.asarray(q, dtype=np.int64)
    return (q >> 31).astype(np.float64), (q & (2 ** 31 - 1)).astype(np.float64)


def profile_join(hi, lo):
    """the int64 sum from the summed halves of profile_split"""
    return (np.asarray(hi, dtype=np.int64) << 31) + np.asarray(lo, dtype=np.int64)


def profile_normalise(count, sums, exponents, nbins, volume, boltz, mvv2e, mv2d, com):
    """compute profile/mdp's array [rows][ndim + 7] from rank-summed integer tables (DeviceDomain.profile_read): the bin centre
    in each named dimension in reduced units (the first slowest), count, density/number, density/mass, temp and the three
    components of the bin's centre-of-mass velocity.  volume: of the whole box; com: temp from the kinetic energy about the
    bin's centre-of-mass velocity.  An empty bin reads 0 in every value column."""
    nbins = [int(n) for n in np.atleast_1d(nbins)]
    rows, ndim = int(np.prod(nbins)), len(nbins)
    count = np.asarray(count, dtype=np.float64).reshape(rows)
    t = np.ldexp(np.asarray(sums, dtype=np.int64).reshape(rows, capi.PROFILE_W).astype(np.float64), -np.asarray(exponents, dtype=np.int32))
    out = np.zeros((rows, ndim + 7))
    idx = np.unravel_index(np.arange(rows), nbins)
    for k in range(ndim):
        out[:, k] = (idx[k] + 0.5) / nbins[k]
    vbin = volume / rows
    full = count > 0
    msum, p, kin = t[:, 0], t[:, 1:4], t[:, 4]
    safe_m = np.where(msum > 0.0, msum, 1.0)
    if com:
        kin = kin - (p ** 2).sum(axis=1) / safe_m
    out[:, ndim] = count
    out[:, ndim + 1] = count / vbin
    out[:, ndim + 2] = np.where(full, mv2d * msum / vbin, 0.0)
    out[:, ndim + 3] = np.where(full, mvv2e * kin / (3.0 * np.where(full, count, 1.0) * boltz), 0.0)
    out[:, ndim + 4:] = np.where(full[:, None], p / safe_m[:, None], 0.0)
    return out


class DeviceDomain:
    """One brick of the periodic box per GPU, all bookkeeping on the device.

    s: the GLOBAL system (every rank builds the same synthetic system and keeps the atoms of its brick --
    setup only; nothing global exists afterwards).  transport=None: one GPU, no communication."""

    def __init__(self, ctx: capi.Context, style: int, s: S.System, cutghost: float, skin: float, map_, v0=None,
                 dt: float = 0.001, transport: Transport | None = None, master_list: bool = False,
                 self_remote: bool = False, nonperiodic=(0, 0, 0)):
        from . import decomp
        self.ctx, self.style, self.box, self.skin, self.dt = ctx, style, s.box, skin, dt
        self.tr = transport
        self.world = 1 if transport is None else transport.world
        self.rank = 0 if transport is None else transport.rank
        self.grid = decomp.proc_grid(self.world)
        self.natoms_total = s.n
        self._mass_by_type = np.array(s.mass, dtype=np.float64)
        # (dimensions that are not periodic -- a slab, a free surface -- are neither wrapped nor given images)
        lam0 = s.box.x2lamda(s.x)
        per = np.array([0.0 if nonperiodic[d] else 1.0 for d in range(3)])
        xw = np.ascontiguousarray(s.box.lamda2x(lam0 - np.floor(lam0) * per))
        if self.world > 1:
            g = np.array(self.grid)
            lam = s.box.x2lamda(xw)
            cell = np.clip(np.floor(lam * g).astype(np.int64), 0, g - 1)
            mine = ((cell[:, 0] * g[1] + cell[:, 1]) * g[2] + cell[:, 2]) == self.rank
        else:
            mine = np.ones(s.n, dtype=bool)
        x = np.ascontiguousarray(xw[mine])
        v = np.zeros_like(x) if v0 is None else np.ascontiguousarray(np.asarray(v0, dtype=np.float64)[mine])
        cfg = capi.MdConfig()
        cfg.style, cfg.nlocal, cfg.nghost, cfg.ntypes = style, len(x), 0, len(s.mass) - 1
        cfg.skin, cfg.dt, cfg.ftm2v, cfg.mvv2e = skin, dt, S.FTM2V, S.MVV2E
        cfg.master_list = 1 if master_list else 0
        cfg.nghost_self = 0
        corners = s.box.lamda2x(np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=float))
        for d in range(3):   # provisional: the library sets the bounds of the brick at every reneighboring
            cfg.bbox_lo[d], cfg.bbox_hi[d] = corners[:, d].min() - cutghost - 2.0, corners[:, d].max() + cutghost + 2.0
        e3, e1 = np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
        if transport is not None and not transport.stage_host and not getattr(transport, "native", False):
            # pack -> all_to_all -> unpack are only ordered when the context launches on the stream the
            # collectives synchronise with (torch's current stream)
            ctx.set_stream(transport.torch.cuda.current_stream().cuda_stream)
        ctx.md_setup(cfg, x, v, s.type[mine], s.tag[mine], s.mass, map_, e1, e3, e1, e1)
        ctx.dd_setup(s.box, self.grid, self.rank, cutghost, self_remote=self_remote, nonperiodic=nonperiodic)
        self.native = bool(getattr(transport, "native", False))
        self.native_two_call = True    # (False: the library's transport through the piecewise calls below -- tests)
        if self.native:
            transport.attach(ctx)
        self.send3 = self.recv3 = self.send1 = self.recv1 = None
        self.builds = 0
        self.dangerous = 0
        self.aeam_overlapped = 0       # multi-GPU aeam steps whose exchanges travelled behind the interior tiles
        self._final_pending = False
        self._nbath = 0                # baths set through langevin_baths (0: langevin() or none), and the one bath's bit
        self._bath_bit = 0
        self.reneighbor()

    # ------------------------------------------------------------------ reneighboring
    def reneighbor(self):
        """Comm::exchange + Comm::borders + Neighbor::build, per rank on the device"""
        self.flush()
        ctx, tr = self.ctx, self.tr
        if tr is None:
            ctx.dd_reneighbor()
        elif self.native:
            ctx.dd_comm_reneighbor()
        else:
            torch = tr.torch
            f64 = dict(dtype=torch.float64, device=tr.device)
            sc = ctx.dd_migrate_begin()
            rc = tr.counts(sc)
            if _os.environ.get("MDP_DIAG"):
                print(f"[dd diag] rank {self.rank} reneighbor {self.builds}: nlocal {ctx.dd_info()['nlocal']} "
                      f"leave {sc.tolist()} arrive {rc.tolist()}", flush=True)
            send = torch.empty(max(int(sc.sum()) * 8, 1), **f64)
            ctx.dd_migrate_pack(send.data_ptr())
            recv, _ = tr.exchange(send, sc, rc, 8)
            if not tr.stage_host:
                torch.cuda.current_stream().synchronize()
            ctx.dd_migrate_end(int(rc.sum()), recv.data_ptr())
            sc = ctx.dd_borders_begin()
            rc = tr.counts(sc)
            send = torch.empty(max(int(sc.sum()) * 6, 1), **f64)
            ctx.dd_borders_pack(send.data_ptr())
            recv, _ = tr.exchange(send, sc, rc, 6)
            ctx.dd_borders_end(rc, recv.data_ptr())
            ctx.md_build_neighbors()
            self.send_counts, self.recv_counts = sc, rc
            ns, nr = int(sc.sum()), int(rc.sum())
            self.send3 = torch.empty(max(ns, 1) * 3, **f64)
            self.recv3 = torch.empty(max(nr, 1) * 3, **f64)
            self.send1 = torch.empty(max(ns, 1), **f64)
            self.recv1 = torch.empty(max(nr, 1), **f64)
            if self.style == capi.STYLE_AEAM:   # the reverse exchange of a step travels beside the fp exchange
                self.rsend3 = torch.empty(max(nr, 1) * 3, **f64)
                self.rrecv3 = torch.empty(max(ns, 1) * 3, **f64)
            self._keep = (send, recv)   # until the stream has consumed them
        info = ctx.dd_info()
        self.nlocal, self.nself, self.nsend, self.nrecv = info["nlocal"], info["nself"], info["nsend"], info["nrecv"]
        self.nghost = self.nself + self.nrecv
        self.builds += 1
        self.fresh_ghosts = True
        # Whether a step exchanges anything is decided for ALL ranks alike, once per reneighboring: every exchange is a
        # collective over the whole group, so a rank without neighbours of its own (a brick facing vacuum across
        # non-periodic faces) takes part with empty messages as long as any rank has a halo.
        self.halo_active = tr.any(bool(self.nsend or self.nrecv)) if tr is not None else False
        if self.style == capi.STYLE_AEAM and tr is not None:
            # ghost forces are non-zero only when some rank has an angular centre next to a remote ghost: the reverse
            # exchange is skipped by all ranks alike otherwise (decided once per reneighboring)
            self.ghost_forces = tr.any(ctx.md_aeam_state()["ghost_forces"])

    @property
    def tags_local(self):
        return self.ctx.md_download_int("tag", self.nlocal)

    # ------------------------------------------------------------------ halo
    def _active(self):
        return self.tr is not None and self.halo_active

    def forward_positions(self, async_op=False):
        if self.native:
            self.ctx.dd_comm_forward_begin()      # exchange in flight on the library's communication stream
            if async_op:
                return "native"
            self.ctx.dd_comm_forward_end()
            return None
        self.ctx.dd_forward_pack(self.send3.data_ptr())
        _, w = self.tr.exchange(self.send3, self.send_counts, self.recv_counts, 3, recv=self.recv3, async_op=async_op)
        if async_op:
            return w
        self.ctx.dd_forward_unpack(self.recv3.data_ptr())

    def forward_fp(self):
        if self.native:
            self.ctx.dd_comm_forward_scalar()
            return
        self.ctx.dd_forward_scalar_pack(self.send1.data_ptr())
        self.tr.exchange(self.send1, self.send_counts, self.recv_counts, 1, recv=self.recv1)
        self.ctx.dd_forward_scalar_unpack(self.recv1.data_ptr())

    def reverse_forces(self, remote=True):
        """ghost forces back to their owners.  remote=False: only the rank's own periodic images are folded -- the
        caller knows (collectively, `ghost_forces`) that no rank put a force on a remote ghost."""
        if self.native:
            if remote:
                self.ctx.dd_comm_reverse()        # folds the self-images too
            else:
                self.ctx.md_fold_self_ghost_f()
            return
        self.ctx.md_fold_self_ghost_f()
        if not remote or not self._active():
            return
        self.ctx.dd_reverse_pack(self.recv3.data_ptr())
        self.tr.exchange(self.recv3, self.recv_counts, self.send_counts, 3, recv=self.send3)
        self.ctx.dd_reverse_unpack(self.send3.data_ptr())

    # ------------------------------------------------------------------ MD
    def compute(self, eflag=0, vflag=0):
        """Pair::compute for the current positions (ghosts must be current)"""
        self.flush()
        if self.style == capi.STYLE_REBOMOS or not self._active():
            self.ctx.md_compute(eflag, vflag)
            return
        self.ctx.md_aeam_density(eflag)
        self.forward_fp()
        self.ctx.md_aeam_force(eflag, vflag)
        self.reverse_forces()

    def flush(self):
        """the final_integrate a step(defer_final=True) left to the next step's fused kernel, now (before anything
        that reads the velocities or replaces the forces)"""
        if self._final_pending:
            self.ctx.md_final_integrate()
            self._final_pending = False

    def _aeam_step_compute(self, eflag, vflag, fresh):
        """Pair::compute of a multi-GPU aeam step in four phases (mdpair_hip.h): the position exchange travels behind
        the density of the interior tiles, the style's fp exchange (pair_aeam.cpp:307) and the reverse exchange of the
        three-body forces on ghosts behind the pair forces of the interior tiles."""
        ctx, tr = self.ctx, self.tr
        work = None if fresh else self.forward_positions(async_op=True)
        ctx.md_compute_begin(eflag, vflag)                       # A: density, interior tiles
        if not fresh:
            if self.native:
                ctx.dd_comm_forward_end()
            else:
                if work not in (None, "native"):
                    work.wait()
                ctx.dd_forward_unpack(self.recv3.data_ptr())
        ctx.md_aeam_density(eflag)                               # B: the rest of passes 1 + 2 (+ three-body forces)
        rev = self.ghost_forces
        if not ctx.md_aeam_state()["phase"] & 4:                 # phase A did not run (pruning due, CSR lists, ...)
            # That is THIS rank's business (its own rows are due for pruning): the peers may be on the phased order in
            # the same step, so the exchanges issued here are exactly theirs, in their order -- fp forward, then the
            # ghost forces back iff `ghost_forces` says any rank has some (decided collectively per reneighboring).
            self.forward_fp()
            ctx.md_aeam_force(eflag, vflag)
            self.reverse_forces(remote=rev)
            return
        self.aeam_overlapped += 1
        if self.native:
            ctx.dd_comm_aeam_exchange_begin(rev)                 # fp out, ghost forces back: one group of sends
            ctx.md_aeam_force_begin(eflag, vflag)                # C: pair forces, interior tiles
            ctx.dd_comm_aeam_exchange_end()
            ctx.md_aeam_force(eflag, vflag)                      # D: the rest
            return
        ctx.md_fold_self_ghost_f()
        ctx.dd_forward_scalar_pack(self.send1.data_ptr())
        if rev:
            ctx.dd_reverse_pack(self.rsend3.data_ptr())
        _, w1 = tr.exchange(self.send1, self.send_counts, self.recv_counts, 1, recv=self.recv1, async_op=True)
        w3 = None
        if rev:
            _, w3 = tr.exchange(self.rsend3, self.recv_counts, self.send_counts, 3, recv=self.rrecv3, async_op=True)
        ctx.md_aeam_force_begin(eflag, vflag)                    # C
        if w1 is not None:
            w1.wait()
        ctx.dd_forward_scalar_unpack(self.recv1.data_ptr())
        ctx.md_aeam_force(eflag, vflag)                          # D
        if rev:
            if w3 is not None:
                w3.wait()
            ctx.dd_reverse_unpack(self.rrecv3.data_ptr())

    def step(self, eflag=0, vflag=0, rebuild=False, defer_final=False):
        """one velocity-Verlet step, Verlet::run order: initial_integrate, [reneighbor], forward comm, force,
        final_integrate.  REBO-MoS on several GPUs hides the ghost exchange behind the interior Lennard-Jones work.
        defer_final: leave this step's final_integrate to the next step, whose first kernel then does both
        half-kicks in one pass (mdp_md_final_initial_integrate; same arithmetic) -- for steps after which nothing
        reads the velocities; thermo() / compute() / reneighbor() / flush() complete it otherwise."""
        ctx = self.ctx
        if self.native and self.tr is not None and self.native_two_call:
            # The library's own transport drives the whole step in two calls (mdp_dd_comm_step_begin / _end): integrate,
            # decide, reneighbor or exchange, compute, final kick.  rebuild="halo" (or "auto"): the collective `check yes`
            # decision comes from the word that travelled with the previous step's halo -- no blocking call here.
            force = -1 if isinstance(rebuild, str) else (1 if rebuild else 0)
            ren = ctx.dd_comm_step_begin(self._final_pending, force, eflag, vflag)
            self._final_pending = False
            if ren:
                info = ctx.dd_info()
                self.nlocal, self.nself, self.nsend, self.nrecv = info["nlocal"], info["nself"], info["nsend"], info["nrecv"]
                self.nghost = self.nself + self.nrecv
                self.builds += 1
            ctx.dd_comm_step_end(eflag, vflag, defer_final)
            self._final_pending = bool(defer_final)
            si = ctx.dd_comm_step_info()
            self.aeam_overlapped, self.ghost_forces, self.dangerous = si["aeam_phased"], si["ghost_forces"], si["dangerous"]
            self.overlap_policy = si["overlap_policy"]
            return
        if isinstance(rebuild, str):        # "auto": one GPU, deferred on-device flag read every step
            if self.tr is not None:
                raise ValueError("rebuild='auto' is for one-GPU runs; the torch / thread transports decide collectively "
                                 "(needs_rebuild); the library's transport takes rebuild='halo'")
            rebuild, late = ctx.md_integrate_check(self._final_pending)   # integrate + check in one pass
            self.dangerous += int(late)
        elif self._final_pending:
            ctx.md_final_initial_integrate()
        else:
            ctx.md_initial_integrate()
        self._final_pending = False
        if rebuild:
            self.reneighbor()               # the border exchange carries the current positions
        fresh, self.fresh_ghosts = self.fresh_ghosts and rebuild, False
        if not self._active():
            ctx.md_compute(eflag, vflag)
        elif self.style == capi.STYLE_REBOMOS:
            work = None if fresh else self.forward_positions(async_op=True)   # pack + all-to-all in flight
            ctx.md_compute_begin(eflag, vflag)
            if not fresh:
                if self.native:
                    ctx.dd_comm_forward_end()
                else:
                    if work is not None:
                        work.wait()
                    ctx.dd_forward_unpack(self.recv3.data_ptr())
            ctx.md_compute_end(eflag, vflag)
        else:
            self._aeam_step_compute(eflag, vflag, fresh)
        if defer_final:
            self._final_pending = True
            ctx.md_defer_final()        # (the library completes the kick itself if velocities are read before the next step)
        else:
            ctx.md_final_integrate()

    def set_group(self, mask_by_tag, integrate_bit, langevin_bit=0):
        """LAMMPS groups for the integrate calls of this domain: mask_by_tag[t] is atom->mask of the atom with tag t (an
        integer array indexed by tag; bit 1 on every atom, as in LAMMPS), integrate_bit the group bit of the integrating
        fix -- every other atom keeps x and v bit for bit --, langevin_bit that of the Langevin thermostat (0: all of the
        integrate group).  The mask then travels with the atoms (reneighborings, migration).  mask_by_tag=None
        withdraws the mask and both groups.  With several ranks every rank makes the same call.  Baths set through
        langevin_baths keep the bits they were given: with several on, a non-zero langevin_bit is refused; with one on,
        langevin_bit=0 leaves that bath's bit in place."""
        self.flush()
        several = self._nbath > 1
        if several and langevin_bit:
            raise ValueError(f"set_group: {self._nbath} Langevin baths are on (langevin_baths); each has the bit it was given")
        if mask_by_tag is None:
            self.ctx.integrate_group(0)
            if not several:
                self.ctx.langevin_group(0)
                self._bath_bit = 0
            self.ctx.md_set_mask(None)
            return
        m = np.asarray(mask_by_tag)
        tags = self.tags_local
        self.ctx.md_set_mask(m[tags].astype(np.int32))
        self.ctx.integrate_group(integrate_bit)
        if not several:
            self.ctx.langevin_group(langevin_bit or self._bath_bit)

    def mask_local(self):
        """the owned atoms' mask in device order (next to tags_local)"""
        return self.ctx.md_download_int("mask", self.nlocal)

    # ------------------------------------------------------------------ image flags and the mean-squared displacement
    def track_images(self, image_by_tag=None):
        """LAMMPS image flags for the atoms of this domain: image_by_tag[t - 1] is atom->image (the 32-bit imageint) of the
        atom with tag t; None: every atom starts in the central image.  From here on every reneighbouring counts the
        box vectors it takes off an atom, and the flag travels with the atom (re-ordering, migration, the minimiser's
        reneighbourings).  With several ranks every rank makes the same call."""
        tags = self.tags_local
        if image_by_tag is None:
            img = np.full(self.nlocal, IMAGE0, dtype=np.int32)
        else:
            img = np.asarray(image_by_tag)[tags - 1].astype(np.int32)
        self.ctx.md_set_image(img)

    def images_local(self):
        """the owned atoms' image counts (ix, iy, iz) [nlocal][3] in device order (next to tags_local)"""
        return image_counts(self.ctx.md_download_int("image", self.nlocal))

    def unwrapped_local(self):
        """the owned atoms' unwrapped positions x + h . image in device order"""
        return self.ctx.md_download_unwrapped(self.nlocal)

    def _group_sum(self, values):
        return np.asarray(values, dtype=np.float64) if self.tr is None else np.asarray(self.tr.sum(values))

    def msd(self, x0_by_tag=None, group_bit=0):
        """starts a mean-squared displacement measurement (LAMMPS compute msd) over the atoms with mask & group_bit (0:
        every atom; otherwise set_group must have given a mask).  x0_by_tag[t - 1]: the unwrapped origin of the atom with
        tag t, for all atoms of the system; None: where the atoms are now.  Needs track_images.  With several ranks every
        rank makes the same call."""
        n = self.natoms_total
        if x0_by_tag is None and self.tr is not None:
            x0 = np.zeros((n, 3))            # every rank fills in its own atoms; the sum is the whole system by tag
            x0[self.tags_local - 1] = self.unwrapped_local()
            x0_by_tag = self._group_sum(x0.ravel()).reshape(n, 3)
        self.ctx.msd_setup(n, x0_by_tag, group_bit)
        # the group's centre of mass at the origins: mass and membership do not change, so it is the sum over the atoms
        # each rank holds now
        m = self._mass_local()
        if group_bit:
            m = m * ((self.mask_local() & group_bit) != 0)
        x0 = self.unwrapped_local() if x0_by_tag is None else np.asarray(x0_by_tag, dtype=np.float64)[self.tags_local - 1]
        w = self._group_sum([*(m[:, None] * x0).sum(axis=0), m.sum()])
        if not w[3] > 0.0:
            raise ValueError("msd: the group holds no atom")
        self._msd_cm0 = w[:3] / w[3]

    def _mass_local(self):
        return np.asarray(self._mass_by_type)[self.ctx.md_download_int("type", self.nlocal)]

    def msd_read(self, com=False):
        """the four values of LAMMPS compute msd -- dx^2, dy^2, dz^2 and their total, means over the group, summed over the
        ranks through the domain's transport.  com: with the drift of the group's centre of mass taken out (com yes)."""
        self.flush()
        shift = None
        if com:
            w = self._group_sum(self.ctx.msd_sums())
            shift = w[4:7] / w[7] - self._msd_cm0
        s = self._group_sum(self.ctx.msd_sums(shift))
        v = s[:3] / s[3]
        return np.array([v[0], v[1], v[2], v[0] + v[1] + v[2]])

    def msd_off(self):
        self.ctx.msd_off()

    # ------------------------------------------------------------------ g(r) and coordination numbers
    def rdf(self, nbin, cutoff, pairs, member_by_tag=None):
        """starts a pair-distance histogram (LAMMPS compute rdf) of nbin bins below cutoff (at most cutghost - skin: what the
        ghost shell guarantees between two reneighbourings).  pairs: one (itype, jtype) per column, each a LAMMPS type or an
        inclusive range (lo, hi).  member_by_tag[t - 1] non-zero: the atom with tag t is in the group, for all atoms of the
        system; None: every atom.  With several ranks every rank makes the same call."""
        rng = lambda t: (int(t), int(t)) if np.ndim(t) == 0 else (int(t[0]), int(t[1]))
        self._rdf = dict(nbin=int(nbin), cutoff=float(cutoff), pairs=[rng(i) + rng(j) for i, j in pairs])
        self.ctx.rdf_setup(nbin, cutoff, self._rdf["pairs"], member_by_tag)

    def rdf_read(self):
        """(hist[npair][nbin], icount[npair], jcount[npair], dup[npair]) as int64, summed over the ranks through the domain's
        transport; rdf_normalise makes LAMMPS' array of them"""
        self.flush()
        hist, ic, jc, du = self.ctx.rdf_counts()
        flat = np.concatenate([hist.ravel(), ic, jc, du])
        assert int(flat.max(initial=0)) < 2 ** 53          # (the transports sum doubles: exact below 2^53)
        tot = np.rint(self._group_sum(flat.astype(np.float64))).astype(np.int64)
        nh, npair = hist.size, len(ic)
        return (tot[:nh].reshape(hist.shape), tot[nh:nh + npair], tot[nh + npair:nh + 2 * npair], tot[nh + 2 * npair:])

    def rdf_off(self):
        self.ctx.rdf_off()

    # ------------------------------------------------------------------ bond-angle distributions
    def adf(self, nbin, triples, ordinate="degree", member_by_tag=None):
        """starts a bond-angle histogram (LAMMPS compute adf) of nbin bins.  triples: one (itype, jtype, ktype, rjin, rjout,
        rkin, rkout) per pair of columns, each type a LAMMPS type or an inclusive range (lo, hi), the outer radii at most
        cutghost - skin.  ordinate: degree, radian or cosine.  member_by_tag as in rdf.  With several ranks every rank makes
        the same call."""
        rng = lambda t: (int(t), int(t)) if np.ndim(t) == 0 else (int(t[0]), int(t[1]))
        rows = [rng(t[0]) + rng(t[1]) + rng(t[2]) + tuple(float(r) for r in t[3:7]) for t in triples]
        self._adf = dict(nbin=int(nbin), ordinate=ordinate, triples=rows)
        self.ctx.adf_setup(nbin, ordinate, rows, member_by_tag)

    def adf_read(self):
        """(hist[ntriple][nbin], icount[ntriple]) as int64, summed over the ranks through the domain's transport;
        adf_normalise makes the compute's array of them"""
        self.flush()
        hist, ic = self.ctx.adf_counts()
        flat = np.concatenate([hist.ravel(), ic])
        assert int(flat.max(initial=0)) < 2 ** 53          # (the transports sum doubles: exact below 2^53)
        tot = np.rint(self._group_sum(flat.astype(np.float64))).astype(np.int64)
        return tot[:hist.size].reshape(hist.shape), tot[hist.size:]

    def adf_off(self):
        self.ctx.adf_off()

    # ------------------------------------------------------------------ per-atom structure
    def coord(self, cutoff, jtypes=None, group_bit=0):
        """starts per-atom coordination numbers (LAMMPS compute coord/atom cutoff): for every owned atom with mask & group_bit
        (0: every atom; otherwise set_group must have given a mask) the atoms of any group inside cutoff (at most cutghost -
        skin), one column per entry of jtypes, each a LAMMPS type or an inclusive range (lo, hi); None: one column over all
        types.  With several ranks every rank makes the same call."""
        rng = lambda t: (int(t), int(t)) if np.ndim(t) == 0 else (int(t[0]), int(t[1]))
        cols = [(1, len(self._mass_by_type) - 1)] if jtypes is None else [rng(t) for t in jtypes]
        self.ctx.coord_setup(cutoff, cols, group_bit)

    def coord_read(self):
        """(tags[nlocal], values[nlocal][ncol]) of this rank's owned atoms; 0 for an atom outside the group"""
        self.flush()
        return self.ctx.coord_read(self.nlocal)

    def coord_off(self):
        self.ctx.coord_off()

    def centro(self, nnn, cutoff=None, group_bit=0):
        """starts the per-atom centro-symmetry parameter (LAMMPS compute centro/atom): nnn "fcc" (12), "bcc" (8) or an even
        number; for every owned atom of the group the nnn nearest atoms inside cutoff (None: cutghost - skin), the nnn / 2
        smallest |R_a + R_b|^2 of their pairs added.  An atom with fewer than nnn atoms inside gets 0."""
        self.ctx.centro_setup(nnn, cutoff, group_bit)

    def centro_read(self):
        """(tags[nlocal], values[nlocal]) of this rank's owned atoms; ctx.centro_info()["few"]: the atoms short of nnn neighbours"""
        self.flush()
        return self.ctx.centro_read(self.nlocal)

    def centro_off(self):
        self.ctx.centro_off()

    def cna(self, cutoff, group_bit=0):
        """starts the per-atom common neighbour analysis (LAMMPS compute cna/atom cutoff): for every owned atom of the group the
        pattern of its neighbours inside cutoff (at most cutghost - skin): 1 fcc, 2 hcp, 3 bcc, 4 icosahedral, 5 other"""
        self.ctx.cna_setup(cutoff, group_bit)

    def cna_read(self):
        """(tags[nlocal], values[nlocal]) of this rank's owned atoms; ctx.cna_counts(): this rank's census of the read,
        ctx.cna_info()["over"]: the atoms with more than 16 neighbours"""
        self.flush()
        return self.ctx.cna_read(self.nlocal)

    def cna_off(self):
        self.ctx.cna_off()

    # ------------------------------------------------------------------ temperature, density and flow profiles
    def profile(self, dims, nbins, group_bit=0):
        """starts a binned measurement of mass, momentum and kinetic energy (LAMMPS compute chunk/atom bin/1d|2d|3d with
        temp/chunk and vcm/chunk): bins over the box in the distinct dimensions dims (0, 1, 2; the first slowest) with
        nbins[k] bins each, over the atoms with mask & group_bit (0: every atom; otherwise set_group must have given a
        mask).  With several ranks every rank makes the same call."""
        self._profile = dict(dims=[int(d) for d in np.atleast_1d(dims)], nbins=[int(n) for n in np.atleast_1d(nbins)])
        self.ctx.profile_setup(self._profile["dims"], self._profile["nbins"], group_bit)

    def profile_read(self):
        """(count[rows], sums[rows][5], exponents[5]): the atoms per bin and the sums of llrint(t_k 2^exponents[k]) over them,
        t = (m, m vx, m vy, m vz, m v.v), as int64 summed over the ranks; profile_normalise makes the compute's array of
        them.  Exact: the exponents come from the global maximum of |t_k|, so every rank rounds alike and the integer sums
        do not depend on the decomposition."""
        self.flush()
        w = capi.PROFILE_W
        slots = np.zeros((self.world, w))            # a maximum through the transports' sum: every rank fills its own slot
        slots[self.rank] = self.ctx.profile_range()
        gmax = self._group_sum(slots.ravel()).reshape(self.world, w).max(axis=0)
        ex = [self.ctx.profile_exponent(r, self.natoms_total) for r in gmax]
        count, sums = self.ctx.profile_sums(ex)
        if self.tr is not None:
            # the transports add doubles: an int64 travels as q >> 31 and q & (2^31 - 1), each sum exact below 2^53
            hi, lo = profile_split(sums)
            flat = np.concatenate([count.astype(np.float64), hi.ravel(), lo.ravel()])
            tot = np.rint(self._group_sum(flat)).astype(np.int64)
            n = count.size
            count = tot[:n]
            sums = profile_join(tot[n:n + sums.size], tot[n + sums.size:]).reshape(sums.shape)
        return count, sums, np.array(ex, dtype=np.int32)

    def profile_off(self):
        self.ctx.profile_off()

    # ------------------------------------------------------------------ the heat current
    def heatflux(self, group_bit=0):
        """LAMMPS compute heat/flux's six values -- J = sum (ke + pe) v + sum W.v, then its convective part sum (ke + pe) v --
        over the atoms with mask & group_bit (0: every atom), summed over the ranks through the domain's transport; extensive,
        not divided by the volume.  The last step (or compute) must have run with eflag | 2 and vflag | 4."""
        self.flush()
        s = self._group_sum(self.ctx.heatflux_sums(group_bit))
        return np.concatenate([s[0:3] + s[3:6], s[0:3]])

    def thermostat(self, t_start, t_stop, t_period, tchain=3, tloop=1, drag=0.0, first=0, last=0, nf=None):
        """Nose-Hoover chain thermostat (LAMMPS fix nvt) in the integrate calls of this domain, from the chain at rest; one
        GPU only.  first / last: the ramp of the run that follows (nhc_run).  nf: the degrees of freedom, 3 N - 3 of all
        atoms unless given -- with an integrate group (set_group) 3 N_group - 3."""
        if self.world > 1:
            raise ValueError("the thermostat runs on one GPU only (multi-rank NVT would need a per-step all-reduce)")
        self.ctx.nhc_setup(t_start, t_stop, t_period, 3.0 * self.natoms_total - 3.0 if nf is None else float(nf), tchain=tchain, tloop=tloop,
                           drag=drag, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        self.ctx.nhc_run(first, last)

    def thermostat_off(self):
        """back to NVE; a deferred final half completes inside mdp_nhc_off, with its chain update"""
        self.ctx.nhc_off()
        self._final_pending = False

    def thermostat_state(self):
        """the chain after the last half-update (completes a deferred final half first)"""
        self.flush()
        return self.ctx.nhc_state()

    def langevin(self, t_start, t_stop, damp, seed, ratio=None, zero=False, tally=False, first=0, last=0, natoms=None):
        """Langevin thermostat (LAMMPS fix langevin, noise keyed by tag and step) in the integrate calls of this domain.
        zero / tally need one GPU.  first / last: the ramp of the run that follows (langevin_run).  natoms: the atoms
        `zero` divides by, all of them unless given -- with a Langevin group (set_group) that group's count."""
        if self.world > 1 and (zero or tally):
            raise ValueError("Langevin zero and tally run on one GPU only (they sum over all atoms every step)")
        self.ctx.langevin_setup(t_start, t_stop, damp, seed, self.natoms_total if natoms is None else int(natoms), ratio=ratio, zero=zero, tally=tally,
                                boltz=S.BOLTZ, mvv2e=S.MVV2E)
        self._nbath = self._bath_bit = 0
        self.ctx.langevin_run(first, last)

    def langevin_baths(self, baths, first=0, last=0):
        """Several Langevin thermostats on disjoint groups in the integrate calls of this domain: baths is a list of
        dicts with the keywords of langevin() (t_start, t_stop, damp, seed, ratio, zero, tally) plus `bit`, the bath's
        group bit in the mask of set_group, and `natoms`, the atoms of that group (`zero` divides by it).  All baths
        share first / last.  The groups must be disjoint and inside the integrate group; one bath is langevin() with
        set_group's langevin_bit.  zero / tally need one GPU."""
        if self.world > 1 and any(b.get("zero") or b.get("tally") for b in baths):
            raise ValueError("Langevin zero and tally run on one GPU only (they sum over all atoms every step)")
        self.flush()
        cfgs = []
        for b in baths:
            b = dict(b)
            b["t_period"] = b.pop("damp")
            b["natoms"] = int(b["natoms"]) if b.get("natoms") is not None else self.natoms_total
            cfgs.append(b)
        self.ctx.langevin_baths(cfgs, boltz=S.BOLTZ, mvv2e=S.MVV2E)
        self._nbath = len(cfgs)
        self._bath_bit = int(cfgs[0]["bit"]) if len(cfgs) == 1 else 0
        self.ctx.langevin_run(first, last)

    def langevin_run(self, first, last):
        """another run (and ramp) of the thermostat that is on; a deferred final half completes inside mdp_langevin_run,
        with the force of the run it belongs to"""
        self.ctx.langevin_run(first, last)
        self._final_pending = False

    def langevin_off(self):
        """back to NVE; a deferred final half completes inside mdp_langevin_off, with its Langevin force"""
        self.ctx.langevin_off()
        self._nbath = self._bath_bit = 0
        self._final_pending = False

    def langevin_tally(self, bath=None):
        """the thermostat energy of the last full step (completes a deferred final half first); with several baths
        their sum in bath order, or that of bath `bath`"""
        self.flush()
        return self.ctx.langevin_tally(bath)

    def _one_gpu(self, what):
        if self.world > 1:
            raise ValueError(f"{what} run on one GPU only (their sums would need an all-reduce per step)")

    def _run_from(self, kind, first):
        """mdp_<kind>_run: a pending final half completes inside the call"""
        getattr(self.ctx, kind + "_run")(first)
        self._final_pending = False

    def heat(self, sources, first=0):
        """Constant-flux heat sources (LAMMPS fix heat) behind the final halves of this domain: sources is a list of up to
        four dicts eflux (energy / time; negative: a sink), nevery, bit -- the source's group bit in the mask of set_group.
        Source k's atoms gain eflux nevery dt of kinetic energy about their centre of mass every nevery steps and keep
        their momentum.  The groups must be disjoint and inside the integrate group; one GPU, no thermostat.  first: the
        step the run that follows starts from (it is never heated itself).  A pending final half completes first."""
        self._one_gpu("heat sources")
        self.ctx.heat_setup(sources, mvv2e=S.MVV2E)
        self.heat_run(first)

    def heat_run(self, first):
        """A further run of the sources set by heat(), from step `first` (LAMMPS' second `run`): the phase of
        step % nevery starts over and step `first` itself is not heated again.  A pending final half completes first,
        WITHOUT the sources -- a host that wants the last step of the run before heated completes it first (flush)."""
        self._run_from("heat", first)

    def heat_state(self, src):
        """source src after the last full step (completes a deferred final half first): capi.Context.heat_state"""
        self.flush()
        return self.ctx.heat_state(src)

    def heat_off(self):
        """back to plain NVE; a deferred final half completes inside mdp_heat_off, with its heat pass"""
        self.ctx.heat_off()
        self._final_pending = False

    def indent(self, indenters, first=0):
        """Indenters (LAMMPS fix indent with `units box`) that push on the atoms of this domain: a list of up to four dicts
        as capi.Context.indent_setup takes them -- shape, k, r, c, and optionally dim, side, vel, bit (the group bit in the
        mask of set_group; 0: every atom).  The centre is c at step `first` and moves by vel dt per step.  The forces the
        domain holds at the call are taken to be the pair style's alone (call it behind compute(), as a fix's setup runs
        behind Verlet::setup).  One GPU; no Nose-Hoover chain, heat sources or minimiser next to them."""
        self._one_gpu("indenters")
        self.ctx.indent_setup(indenters)
        self.indent_run(first)

    def indent_run(self, first):
        """A further run of the indenters set by indent(), from step `first`: the centres start again at c.  A pending
        final half completes first, with its indenter forces; compute() again before the next step."""
        self._run_from("indent", first)

    def indent_state(self, k):
        """indenter k for the current forces (completes a deferred final half first): capi.Context.indent_state"""
        self.flush()
        return self.ctx.indent_state(k)

    def indent_off(self):
        """back to the pair style's forces alone; a deferred final half completes inside mdp_indent_off, with its pass"""
        self.ctx.indent_off()
        self._final_pending = False

    def spring(self, springs, first=0):
        """Tether springs (LAMMPS fix spring tether) on the centres of mass of groups of this domain: a list of up to four
        dicts as capi.Context.spring_setup takes them -- k, r0, c (None for a dimension that takes no part), and optionally
        vel, bit (the group bit in the mask of set_group; 0: every atom).  The tether point is c at step `first` and moves by
        vel dt per step.  The centre of mass is that of the unwrapped positions: the domain needs its image flags
        (track_images).  Call it behind compute(), as indent().  One GPU; no Nose-Hoover chain, heat sources or minimiser next
        to them; indenters and Langevin baths are welcome."""
        self._one_gpu("springs")
        self.ctx.spring_setup(springs)
        self.spring_run(first)

    def spring_run(self, first):
        """A further run of the springs set by spring(), from step `first`: the tether points start again at c.  A pending
        final half completes first, with its spring forces; compute() again before the next step."""
        self._run_from("spring", first)

    def spring_state(self, k):
        """spring k for the current forces (completes a deferred final half first): capi.Context.spring_state"""
        self.flush()
        return self.ctx.spring_state(k)

    def spring_off(self):
        """back to the pair style's forces alone; a deferred final half completes inside mdp_spring_off, with its pass"""
        self.ctx.spring_off()
        self._final_pending = False

    def gforce(self, slots, first=0):
        """Prescribed forces on groups of this domain (LAMMPS fix setforce, addforce and aveforce with constant values): a
        list of up to four dicts as capi.Context.gforce_setup takes them -- kind ("set", "add", "ave"), f (None for a
        dimension that is left alone), and optionally bit (the group bit in the mask of set_group; 0: every atom).  They
        act in list order on an atom's force, behind the indenters and the springs; nothing may share atoms with an "ave"
        in front of it.  An "add" needs the domain's image flags (track_images).  Call it behind compute(), as indent().
        One GPU; no Nose-Hoover chain, heat sources or minimiser next to them."""
        self._one_gpu("group forces")
        self.ctx.gforce_setup(slots)
        self.gforce_run(first)

    def gforce_run(self, first):
        """A further run of the slots set by gforce(), from step `first`.  A pending final half completes first, with its
        pass; compute() again before the next step."""
        self._run_from("gforce", first)

    def gforce_state(self, k):
        """slot k for the current forces (completes a deferred final half first): capi.Context.gforce_state"""
        self.flush()
        return self.ctx.gforce_state(k)

    def gforce_off(self):
        """back to the pair style's forces alone; a deferred final half completes inside mdp_gforce_off, with its pass"""
        self.ctx.gforce_off()
        self._final_pending = False

    def minimize(self, etol, ftol, maxiter, maxeval, chunk=64, **modify):
        """FIRE minimisation (LAMMPS min_style fire with its defaults; **modify: capi.FIRE_DEFAULTS) of this domain on the
        device, one GPU only; returns the final state (capi.Context.fire_state).  The velocities are zero afterwards
        up to what the last iteration left; the time step of the domain is unchanged.  With an integrate group
        (set_group) only its atoms move: the others are held with their velocities, and the force norm is the group's."""
        if self.world > 1:
            raise ValueError("the minimiser runs on one GPU only (its sums would need an all-reduce per iteration)")
        self.flush()
        ctx = self.ctx
        ctx.fire_setup(etol, ftol, maxiter, maxeval, **modify)
        try:
            left = int(maxiter) + 2        # (the stop code is seen an iteration or two late; extra iterations change nothing)
            while left > 0 and not ctx.fire_iterate(min(chunk, left)):
                left -= min(chunk, left)
            st = ctx.fire_state()
        finally:
            ctx.fire_off()
        self._after_device_reneighbors(st["reneighbors"])
        return st

    def _after_device_reneighbors(self, n):
        """the library reneighboured on its own (the minimiser): the brick's counts as they are now"""
        info = self.ctx.dd_info()
        self.nlocal, self.nself, self.nsend, self.nrecv = info["nlocal"], info["nself"], info["nsend"], info["nrecv"]
        self.nghost = self.nself + self.nrecv
        self.builds += int(n)

    def tune_overlap(self, max_steps=80):
        """library transport: force-only steps until the library's overlap-policy trial has chosen (comm_rccl.hip); returns
        the step info.  Collective: every rank runs the same steps."""
        si = self.ctx.dd_comm_step_info()
        n = 0
        while si["overlap_policy"].startswith("undecided") and n < max_steps:
            self.step(0, 0, rebuild="halo", defer_final=True)
            si = self.ctx.dd_comm_step_info()
            n += 1
        self.flush()
        si["trial_steps"] = n
        return si

    def thermo(self, reduce=True):
        """KE, PE, virial (summed over ranks), T and P of the whole system"""
        self.flush()
        t = self.ctx.md_thermo()
        if self.tr is not None and reduce:
            tot = self.tr.sum([t["ke"], t["pe"], *t["virial"], ])
            t["ke"], t["pe"], t["virial"] = float(tot[0]), float(tot[1]), tot[2:8]
        t["temp"] = S.temperature(t["ke"], self.natoms_total)
        t["press"] = S.pressure(t["ke"], t["virial"], self.natoms_total, self.box.volume)
        return t

    def moved(self) -> bool:
        """deferred `neigh_modify check yes` flag (see mdp_md_moved_async); one GPU only -- several ranks must
        agree on the step they reneighbor at, see needs_rebuild"""
        m, d = self.ctx.md_moved_async()
        self.dangerous += int(d)
        return m

    def needs_rebuild(self, margin: float = 0.0) -> bool:
        """blocking check, collective over the ranks: some owned atom moved more than skin/2 - margin"""
        self.flush()
        t = self.ctx.md_thermo()
        need = t["maxdisp2"] > max(0.5 * self.skin - margin, 0.25 * self.skin) ** 2
        if t["maxdisp2"] > (0.5 * self.skin) ** 2:
            self.dangerous += 1              # (an atom of THIS rank was beyond half the skin already: a late build)
        return self.tr.any(need) if self.tr is not None else need


class ThreadTransport:
    """Rehearsal transport: N ranks as N threads of ONE process, each with its own context on the same GPU.
    A GPU box admits few processes on its card, so this is how the 4- and 8-brick decompositions (migration,
    borders, per-step halo) are exercised on one GPU; the rank code is exactly what runs over RCCL.
    Exchanges are device-to-device copies between the ranks' torch buffers, fenced by thread barriers."""

    class Shared:
        def __init__(self, world):
            import threading
            self.world = world
            # (a timeout: ranks whose exchange schedules diverge fail the test with BrokenBarrierError instead of hanging)
            self.barrier = threading.Barrier(world, timeout=float(_os.environ.get("MDP_THREAD_BARRIER_TIMEOUT", "180")))
            self.slots = [None] * world

    def __init__(self, shared: "ThreadTransport.Shared", rank: int, ctx: capi.Context, device):
        import torch
        self.torch, self.sh, self.rank, self.world, self.ctx, self.device = torch, shared, rank, shared.world, ctx, device
        self.stage_host = True   # every exchange is synchronous (no overlap in the rehearsal)

    def _all(self, value):
        self.sh.barrier.wait()
        self.sh.slots[self.rank] = value
        self.sh.barrier.wait()
        return list(self.sh.slots)

    def counts(self, send_counts):
        allc = self._all(np.asarray(send_counts, dtype=np.int64).copy())
        return np.array([allc[q][self.rank] for q in range(self.world)], dtype=np.int64)

    def exchange(self, send, send_counts, recv_counts, width, recv=None, async_op=False):
        torch = self.torch
        nrecv = int(np.sum(recv_counts)) * width
        if recv is None:
            recv = torch.empty(max(nrecv, 1), dtype=torch.float64, device=self.device)
        self.ctx.sync()                       # my pack kernel has finished
        off = np.concatenate([[0], np.cumsum(np.asarray(send_counts, dtype=np.int64) * width)])
        peers = self._all((send, off))
        at = 0
        for q in range(self.world):
            n = int(recv_counts[q]) * width
            if n:
                src, soff = peers[q]
                recv[at:at + n].copy_(src[int(soff[self.rank]):int(soff[self.rank]) + n])
            at += n
        torch.cuda.synchronize()
        self.sh.barrier.wait()                # nobody reuses a send buffer before every peer has copied
        return recv, None

    def any(self, flag):
        return any(self._all(bool(flag)))

    def sum(self, values):
        return np.sum(np.array(self._all(np.asarray(list(values), dtype=np.float64))), axis=0)


def run_ranks(world: int, fn, device=0, native=False):
    """run fn(rank, make_transport) on `world` threads; make_transport(ctx) gives the rank's ThreadTransport, or --
    native=True -- a NativeTransport: the library's own RCCL transport with `world` ranks.  On one GPU that needs
    MDP_RCCL_LIBRARY to name the test double of tests/native (RCCL itself refuses two ranks on one device).
    Returns the list of results; the first exception of any rank is re-raised."""
    import threading
    import torch
    shared = ThreadTransport.Shared(world)
    out, err = [None] * world, [None] * world
    dev = torch.device("cuda", device)

    def bcast_from(r):
        def bcast(b):                        # rank 0's communicator id to every rank thread
            shared.barrier.wait()
            if r == 0:
                shared.slots[0] = b
            shared.barrier.wait()
            return shared.slots[0]
        return bcast

    def body(r):
        try:
            torch.cuda.set_device(device)
            if native:
                out[r] = fn(r, lambda ctx: NativeTransport(world, r, bcast_from(r)))
            else:
                out[r] = fn(r, lambda ctx: ThreadTransport(shared, r, ctx, dev))
        except BaseException as e:   # noqa: BLE001 -- re-raised below
            err[r] = e
            shared.barrier.abort()

    import os
    old = capi.Context.serialize
    # every rank thread calls the library concurrently (own context, own stream): what a C++ host that drives
    # several GPUs from threads of one process does.  MDP_THREAD_SERIALIZE=1 puts one process-wide lock around the
    # library (debugging aid).
    capi.Context.serialize = os.environ.get("MDP_THREAD_SERIALIZE", "0") != "0"
    try:
        th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        capi.Context.serialize = old
    real = [e for e in err if e is not None and not isinstance(e, threading.BrokenBarrierError)]
    if real or any(e is not None for e in err):
        raise (real[0] if real else [e for e in err if e is not None][0])
    return out
