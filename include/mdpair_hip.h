/*
 * mdpair_hip.h -- C-ABI of libmdpair_hip.so, the MI355X (gfx950) device layer behind the
 * LAMMPS pair styles `rebomos` and `aeam`.
 *
 * This is the "thin C-ABI layer" of the north star: plain pointers and sizes, no C++ or torch
 * types.  Host code (the PairREBOMoS / PairAEAM plugin adapters in lammps-plugins_amd/plugin/,
 * the mini-host, and the Python bench/test harness via ctypes) reaches the HIP kernels only
 * through these entry points.  Every entry point names the reference interface it replaces
 * (paths relative to the upstream repo lammps/lammps-plugins).
 *
 * Two ways to feed the hot path:
 *   host mode     -- what a LAMMPS `Pair::compute()` has in hand: host pointers to atom->x/type/tag
 *                    and the paged NeighList (SURVEY.md 8b "Data handed to compute").
 *   resident mode -- atoms, ghosts, neighbor lists, integrator and thermo all live on the GPU
 *                    (mdp_md_*); used by the mini-host and by bench.py.  Device buffers may be
 *                    owned by the caller (e.g. torch tensors) -- see mdp_md_ptr().
 *
 * All functions return 0 on success or a negative MDP_E* code; mdp_last_error() gives the text.
 * Nothing here falls back to the CPU: without a usable HIP device every call fails.
 */
#ifndef MDPAIR_HIP_H
#define MDPAIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDP_ABI_VERSION 3

enum {
  MDP_OK = 0,
  MDP_EINVAL = -1,    /* bad argument / call order                                   */
  MDP_EHIP = -2,      /* HIP runtime error (text in mdp_last_error)                  */
  MDP_ENOMEM = -3,
  MDP_EOVERFLOW = -4, /* "Neighbor list overflow, boost neigh_modify one" (pair_rebomos.cpp:350) */
  MDP_ENOTIMPL = -5,  /* feature not available                                       */
  MDP_ESTATE = -6     /* potential / atoms / neighbors not set                       */
};

/* eflag / vflag bits follow LAMMPS ev_setup */
#define MDP_EFLAG_GLOBAL 1
#define MDP_EFLAG_ATOM 2
#define MDP_VFLAG_GLOBAL 1 /* explicit pair virial -> virial[6]; set by either VIRIAL_PAIR or VIRIAL_FDOTR */
#define MDP_VFLAG_ATOM 4

typedef struct mdp_ctx mdp_ctx;

/* ---- lifecycle ------------------------------------------------------------------------- */
int mdp_abi_version(void);
int mdp_device_count(void);
int mdp_create(mdp_ctx **ctx, int device);
int mdp_destroy(mdp_ctx *ctx);
const char *mdp_last_error(const mdp_ctx *ctx);
/* bytes of device memory THIS context holds (ctx = NULL: all contexts of the process): EVERY device buffer of the context --
 * lists, work arrays, tables, the domain's, the fixes' and the measurements' -- counted as it is reserved and released, so
 * the contexts' figures add up to the process total and mdp_destroy takes the total back by exactly the context's.  What
 * Pair::memory_usage() should add for the style's device side (the reference reports the lists it holds:
 * pair_rebomos.cpp:1113-1124) */
double mdp_device_bytes(const mdp_ctx *ctx);
/* host arrays are staged through pinned buffers of the context by default.  With MDP_HOST_REGISTER=1 large arrays
 * (atom->x) are page-locked in place instead; a host that opts in must call this before it frees or re-allocates
 * such an array (LAMMPS: when atom->nmax grows).  ptr = NULL releases every registration. */
int mdp_host_release(mdp_ctx *ctx, const void *ptr);
int mdp_set_stream(mdp_ctx *ctx, void *hip_stream); /* run everything on this hipStream_t (default: own stream) */
int mdp_sync(mdp_ctx *ctx);

/* ---- potentials --------------------------------------------------------------------------
 * REBO Mo-S: the 61 scalars of MoS.REBO.set5b after mixing, i.e. the protected members of
 * PairREBOMoS (USER-REBOMOS/pair_rebomos.h:54-60) as filled by read_file
 * (pair_rebomos.cpp:964-1066) and init_one (pair_rebomos.cpp:262-265).  Element 0 = Mo, 1 = S. */
typedef struct {
  double rcmin[2][2], rcmax[2][2], rcmaxsq[2][2];
  double Q[2][2], alpha[2][2], A[2][2], BIJc[2][2], Beta[2][2];
  double b[7][2], bg[7][2], a[4][2];
  double rcLJmin[2][2], rcLJmax[2][2], epsilon[2][2], sigma[2][2];
  double lj1[2][2], lj2[2][2], lj3[2][2], lj4[2][2];
} mdp_rebomos_params;

int mdp_rebomos_set_params(mdp_ctx *ctx, const mdp_rebomos_params *p);
/* replaces PairREBOMoS::read_file (pair_rebomos.cpp:857-1066): 61 scalars, one per non-comment line,
 * then the mixing rules and lj1..lj4.  err receives a message shaped like pair_rebomos.cpp:955-957. */
int mdp_rebomos_read_file(const char *path, mdp_rebomos_params *p, char *err, int errlen);
int mdp_rebomos_params_from_scalars(const double *v61, mdp_rebomos_params *p);

/* AEAM: the spline tables PairAEAM::array2spline builds (USER-AEAM/pair_aeam.cpp:876-942) and
 * the Setfl scalars (pair_aeam.h:66-76).  Tables are dense [table][row 0..nmax][7] doubles with
 * 1-based rows exactly as the reference stores them; type maps are (ntypes+1)^2 / (ntypes+1),
 * 1-based (pair_aeam.cpp:785-871). */
typedef struct {
  int ntypes, nelements, nnonangular;
  int nrhomax, nrmax, nfrho, nrhor, nz2r;
  const int *nrho;       /* [nelements]            */
  const double *drho;    /* [nelements]            */
  const int *nr;         /* [nelements*nelements]  */
  const double *dr;      /* [nelements*nelements]  */
  const double *cut;     /* [nelements*nelements]  */
  const int *type2frho;  /* [ntypes+1]             */
  const int *type2rhor;  /* [(ntypes+1)*(ntypes+1)]*/
  const int *type2z2r;   /* [(ntypes+1)*(ntypes+1)]*/
  const double *frho_spline; /* [nfrho][nrhomax+1][7] */
  const double *rhor_spline; /* [nrhor][nrmax+1][7]   */
  const double *z2r_spline;  /* [nz2r][nrmax+1][7]    */
} mdp_aeam_tables;

int mdp_aeam_set_tables(mdp_ctx *ctx, const mdp_aeam_tables *t);
/* replaces PairAEAM::read_file (pair_aeam.cpp:627-746), file2array (:752-872) and array2spline /
 * interpolate (:876-942).  map[1..ntypes] = element index of each atom type, -1 for NULL. */
typedef struct mdp_aeam_file mdp_aeam_file;
int mdp_aeam_file_read(const char *path, mdp_aeam_file **out, char *err, int errlen);
/* mass[mass_cap]: one per element (a file may define up to 64; call with mass = NULL to learn nelements first) */
int mdp_aeam_file_info(const mdp_aeam_file *f, int *nelements, int *nnonangular, int *nangular, double *mass,
                       int mass_cap, char *names, int nameslen);
int mdp_aeam_file_build(mdp_aeam_file *f, int ntypes, const int *map, mdp_aeam_tables *out); /* out points into f */
void mdp_aeam_file_free(mdp_aeam_file *f);

/* ---- host mode: the data a LAMMPS Pair::compute() holds ---------------------------------
 * replaces the reads of atom->x/type/tag/nlocal/nghost (pair_rebomos.cpp:288-290,370-374;
 * pair_aeam.cpp:141-145).  x is [nall][3] (LAMMPS double** is contiguous), type is 1-based,
 * map[1..ntypes] = element index (REBO-MoS: pair_rebomos.cpp:168-179; AEAM: identity-1). */
int mdp_set_atoms_host(mdp_ctx *ctx, int nlocal, int nghost, const double *x, const int *type, const int *tag,
                       int ntypes, const int *map);
int mdp_set_positions_host(mdp_ctx *ctx, const double *x); /* per step, same nlocal/nghost */
/* One periodic rank: every ghost is an image of an owned atom, and Comm::forward_comm gives it its owner's position
 * plus whole box vectors.  A host that hands over its box -- h = Domain::h = {xprd, yprd, zprd, yz, xz, xy}, before
 * mdp_set_atoms_host and again whenever the box changes (fix npt / deform: before each mdp_set_positions_host) -- lets
 * the library do that on the device: at mdp_set_atoms_host owner (by tag) and image counts of every ghost are derived
 * and checked against the uploaded positions (1e-8 A); if all ghosts pass, mdp_host_ghosts_derived() returns 1 and
 *   - mdp_set_positions_host reads x[0..nlocal) only (the images follow with the box of that step),
 *   - mdp_aeam_density_host accepts fp == NULL (and rho == NULL): fp stays on the device, images included,
 *   - mdp_aeam_force_host accepts fp_all == NULL, folds what the images collected onto their owners itself (the
 *     host's reverse_comm then carries zeros for this style) and adds into f[0..nlocal) / vatom[0..nlocal) only.
 * With a ghost of another rank's atom, without tags, or with MDP_HOST_GHOSTS=upload the answer is 0 and everything is
 * as before.  h == NULL withdraws the box. */
int mdp_set_box_host(mdp_ctx *ctx, const double *h /* [6] or NULL */);
int mdp_host_ghosts_derived(mdp_ctx *ctx);

/* replaces the reads of list->inum/gnum/ilist/numneigh/firstneigh (pair_rebomos.cpp:304-307,
 * pair_aeam.cpp:150-153).  Call when the host has rebuilt its list (neighbor->ago == 0).
 * firstneigh[i] points into LAMMPS' pages; entries are masked with NEIGHMASK here.
 * skin = neighbor->skin: the list was built at r <= cut+skin and stays valid until the next call;
 * the device repacks it (trimmed, coalesced) once per call. */
int mdp_set_neighbors_host(mdp_ctx *ctx, int inum, int gnum, const int *ilist, const int *numneigh,
                           int *const *firstneigh, double skin);
/* replaces the read of neighbor->skin alone.  The REBO-MoS device path derives its own trimmed lists
 * (REBO candidates, Lennard-Jones cluster pair lists) from the positions, as LAMMPS' own GPU/KOKKOS
 * packages do with `neigh yes`; the host's list is requested for API parity and for the ghost shell it
 * implies but its entries are not read, so a rebomos host only reports the skin (at every reneighboring,
 * after mdp_set_atoms_host).  neigh_modify exclusions are therefore not honoured. */
int mdp_set_skin(mdp_ctx *ctx, double skin);
/* guard that goes with mdp_set_skin: the reference iterates the host's entries (pair_rebomos.cpp:304-307, 328-330,
 * 490-495), so exclusions, special_bonds or skip lists change ITS result.  Compares the host's owned-row entry count
 * with the number of geometric pairs inside cutneigh (= sqrt(cutsq)+skin, the host's list cutoff) counted on the
 * device from the atoms last uploaded, and scans a sample of rows for special-bond bits; MDP_EINVAL + message on
 * any difference.  Call at every reneighboring after mdp_set_atoms_host.  MDP_SKIP_LIST_CHECK=1 disables it. */
int mdp_rebomos_check_host_list(mdp_ctx *ctx, int inum, const int *ilist, const int *numneigh, int *const *firstneigh,
                                double cutneigh);
/* rebomos, host mode: 1 = candidates (REBO_neigh, pair_rebomos.cpp:281-352) and Lennard-Jones rows (FLJ, :490-495)
 * are taken from the HOST's full + ghost neighbor list, handed over with mdp_set_neighbors_host (inum + gnum rows,
 * entries masked with NEIGHMASK as the reference does, :328-330) at every reneighboring -- subsets of what the host
 * listed, so `neigh_modify exclude` and special-bond settings act as in the reference instead of stopping the run
 * (mdp_rebomos_check_host_list is then not called).  The device keeps the host's atom order and the host's ghosts
 * (no mdp_set_box_host images, no fix nve/mdp) and pays the upload of the list: ~640 entries per atom at the
 * reference's 13.4 A list cutoff.  Call before mdp_set_atoms_host.  0 (default): lists from the positions. */
int mdp_rebomos_host_list(mdp_ctx *ctx, int on);
/* aeam, host mode: 1 = the style builds its lists on the device from the positions, exactly as rebomos does
 * (bins, tile lists, CSR rows of the angular centres) and the host only reports its skin (mdp_set_skin) at every
 * reneighboring; the device keeps its own Hilbert-sorted copy of the atoms and returns results in the host's order.
 * The host's list is then not read -- flattening its 86 entries per atom on a host thread and uploading them cost
 * more than ten steps per reneighboring at a million atoms -- so, as for rebomos, a list that is not the plain
 * geometric one must be refused: mdp_aeam_check_host_list (per-type-pair cutoffs cut[ti][tj] + skin,
 * pair_aeam.cpp:615-621).  Call before mdp_set_atoms_host.  0 (default) = stream the host's list
 * (mdp_set_neighbors_host), the reference's own data flow (pair_aeam.cpp:150-153). */
int mdp_aeam_device_lists(mdp_ctx *ctx, int on);
int mdp_aeam_check_host_list(mdp_ctx *ctx, int inum, const int *ilist, const int *numneigh, int *const *firstneigh,
                             double skin);
/* same as mdp_set_neighbors_host, from a CSR copy (tests / hosts that already hold a flat list): offset[nall+1] */
int mdp_set_neighbors_csr_host(mdp_ctx *ctx, int nall, const int *numneigh, const long long *offset,
                               const int *neigh, double skin);

/* replaces PairREBOMoS::compute (pair_rebomos.cpp:102-111): REBO_neigh + FREBO + FLJ + virial.
 * f[nlocal][3] and eatom[nlocal] are ACCUMULATED into (LAMMPS zeroes them); forces are complete
 * for owned atoms (owner-computes: nothing is written to ghosts, so the host's reverse_comm adds
 * zeros).  virial[6] is the explicit pair virial (xx,yy,zz,xy,xz,yz) of this rank's owned atoms,
 * to be used with no_virial_fdotr = 1.  vatom[nlocal][6] (vflag & 4) is the per-atom virial in the
 * reference's split (ev_tally halves, v_tally3 thirds, v_tally2 halves: pair_rebomos.cpp:444,554,707-725),
 * complete for owned atoms.  Any of eng/virial/eatom/vatom may be NULL. */
int mdp_rebomos_compute_host(mdp_ctx *ctx, int eflag, int vflag, double *f, double *eng_vdwl, double *virial,
                             double *eatom, double *vatom);

/* replaces PairAEAM::compute (pair_aeam.cpp:110-479) in two halves around the style's own
 * forward_comm (pair_aeam.cpp:307):
 *   density:  passes 1+2 (rho, F, F'); writes fp[0..nlocal) (host) = F'(rho) chain factor the
 *             neighbors need, adds the embedding energy to *eng_vdwl / eatom.
 *   force:    pass 3; fp_all[nall] must hold the owners' values on ghosts (after forward_comm).
 *             f[nall][3] is accumulated into: owned atoms fully, ghosts only with the angular
 *             three-body terms (folded by the host's reverse_comm).  vatom[nall][6] (vflag & 4, may be
 *             NULL) follows ev_tally / ev_tally3 (pair_aeam.cpp:393,472): halves / thirds, ghosts as for f.
 * With mdp_host_ghosts_derived() == 1 fp / rho / fp_all may be NULL (see mdp_set_box_host): no fp round trip. */
int mdp_aeam_density_host(mdp_ctx *ctx, int eflag, double *fp, double *rho, double *eng_vdwl, double *eatom);
int mdp_aeam_force_host(mdp_ctx *ctx, int eflag, int vflag, const double *fp_all, double *f, double *eng_vdwl,
                        double *virial, double *eatom, double *vatom);

/* ---- resident mode: device-side MD around the hot path -------------------------------------
 * (neighbor build, integrator, thermo.)  One sub-domain per context. */
typedef struct {
  int style;          /* 1 = rebomos, 2 = aeam                                         */
  int nlocal, nghost; /* owned atoms, ghost atoms (periodic self-images + remote halo) */
  int ntypes;
  double skin;
  double dt;
  double ftm2v, mvv2e;   /* unit constants (metal: SURVEY.md Appendix B)               */
  double bbox_lo[3], bbox_hi[3]; /* Cartesian bounds of owned+ghost atoms, for binning  */
  int nghost_self;    /* ghosts [0,nghost_self) are periodic self-images (refreshed on the device), the rest are
                         remote atoms filled by mdp_md_unpack_x; lists that reach none of the latter need not
                         wait for the halo (mdp_md_compute_begin / _end)                                   */
  int master_list;    /* 1 = also build the LAMMPS-style full list of every owned atom (rebomos: at 3*rcmax+skin,
                         log.rebomos-bulk.1:43; aeam: per-type-pair cutoffs + skin, 86 entries/atom) for its
                         statistics.  By default rebomos builds none (its kernels use the style's own lists) and
                         aeam with tile lists builds the rows of the angular centres only; a per-atom-virial step
                         (CSR kernels) switches the full aeam list on by itself.                              */
} mdp_md_config;

/* upload a sub-domain.  x/v/type/tag: owned atoms [nlocal]; ghosts: ghost_owner[g] = local index
 * of the owner (>=0: periodic self-image, refreshed on the device each step) or -1 (remote: filled
 * by mdp_md_unpack_ghosts), ghost_shift[g][3] Cartesian image shift, ghost_type/tag.
 * mass[1..ntypes].  map as in mdp_set_atoms_host. */
int mdp_md_setup(mdp_ctx *ctx, const mdp_md_config *cfg, const double *x, const double *v, const int *type,
                 const int *tag, const double *mass, const int *map, const int *ghost_owner,
                 const double *ghost_shift, const int *ghost_type, const int *ghost_tag);
/* binned full(+ghost) neighbor list on the device with the cutoffs the style's init_one() returns
 * (pair_rebomos.cpp:244-274, pair_aeam.cpp:615-621) + skin, then the style's repack. */
int mdp_md_build_neighbors(mdp_ctx *ctx);
int mdp_md_initial_integrate(mdp_ctx *ctx); /* fix nve: v += dt/2 f/m; x += dt v; refresh self-image ghosts */
int mdp_md_final_integrate(mdp_ctx *ctx);   /* v += dt/2 f/m */
/* final_integrate of the finished step and initial_integrate of the next in one pass over the atoms (same operations,
 * same order: bit-identical trajectory).  For a host that needs the full-step velocities of the finished step for
 * nothing (no thermo output, no dump at that step): it skips mdp_md_final_integrate there and opens the next step
 * with this call instead of mdp_md_initial_integrate. */
int mdp_md_final_initial_integrate(mdp_ctx *ctx);
/* the host's declaration that it skips mdp_md_final_integrate for the step just computed and will open the next step
 * with mdp_md_final_initial_integrate / mdp_md_integrate_check(with_final).  Until then the velocities on the device
 * are half-step velocities: mdp_md_thermo and a velocity download complete the kick themselves first (and the
 * with_final call that follows then applies only the initial half-kick), so nothing reads half-step values unnoticed. */
int mdp_md_defer_final(mdp_ctx *ctx);
int mdp_md_compute(mdp_ctx *ctx, int eflag, int vflag); /* force_clear + Pair::compute on the device */
/* the same in two halves for multi-GPU runs: _begin needs only owned atoms, self-image ghosts and LAST step's
 * remote ghosts (it runs while this step's halo exchange is in flight: the work whose lists reach no remote
 * ghost -- rebomos: the interior REBO centres; aeam: the density of the interior tiles); _end needs the unpacked
 * halo (aeam: _end is density + force + self-image fold for a host without exchanges of its own; a multi-GPU host
 * calls the four aeam phases below instead). */
int mdp_md_compute_begin(mdp_ctx *ctx, int eflag, int vflag);
int mdp_md_compute_end(mdp_ctx *ctx, int eflag, int vflag);
/* halo plumbing for multi-GPU: pack x (or the AEAM fp) of owned atoms sendlist[n] (+shift) into buf;
 * unpack recv buffers into ghosts [first, first+n).  buf/sendlist/shift are DEVICE pointers. */
int mdp_md_pack_x(mdp_ctx *ctx, int n, const int *d_sendlist, const double *d_shift, double *d_buf);
int mdp_md_unpack_x(mdp_ctx *ctx, int first_ghost, int n, const double *d_buf);
int mdp_md_pack_scalar(mdp_ctx *ctx, int which, int n, const int *d_sendlist, double *d_buf);
int mdp_md_unpack_scalar(mdp_ctx *ctx, int which, int first_ghost, int n, const double *d_buf);
int mdp_md_pack_ghost_f(mdp_ctx *ctx, int first_ghost, int n, double *d_buf);       /* reverse comm */
int mdp_md_unpack_add_f(mdp_ctx *ctx, int n, const int *d_sendlist, const double *d_buf);
int mdp_md_fold_self_ghost_f(mdp_ctx *ctx); /* reverse comm for periodic self-images */
/* AEAM only: compute in phases around the style's own exchanges -- forward_comm of fp (pair_aeam.cpp:307, 946-963)
 * and the host's reverse_comm of the forces that three-body terms put on ghosts (pair_aeam.cpp:462-470):
 *   mdp_md_compute_begin     [optional] density of the tiles that reach no remote ghost | position halo in flight
 *   mdp_md_aeam_density      the remaining density, angular centres, embedding; when _compute_begin did run, also the
 *                            three-body forces (they need the centre's own F' only), so that ghost forces are final
 *   mdp_md_aeam_force_begin  [optional] pair forces of the interior tiles           | fp and ghost forces in flight
 *   mdp_md_aeam_force        the remaining pair forces (three-body forces if not done yet); needs fp on the ghosts
 * Without the optional calls the two others do everything, as before.  eflag / vflag must agree between the phases
 * of one compute.  mdp_md_aeam_state: out[0] = phases done so far in the current compute (bit 1: interior density,
 * bit 2: three-body forces, bit 3: interior forces), [1] = tiles that reach no remote ghost, [2] = tiles,
 * [3] = 1 when an angular centre may have a remote ghost in its row (otherwise no ghost force is ever non-zero and
 * the reverse exchange can be skipped by all ranks alike). */
int mdp_md_aeam_density(mdp_ctx *ctx, int eflag);
int mdp_md_aeam_force_begin(mdp_ctx *ctx, int eflag, int vflag);
int mdp_md_aeam_force(mdp_ctx *ctx, int eflag, int vflag);
int mdp_md_aeam_state(mdp_ctx *ctx, int out[4]);
/* thermo: out[0]=KE(owned), [1]=PE (eng_vdwl of last compute), [2..7]=virial of last compute,
 * [8] = max squared displacement since the last neighbor build (neigh_modify check yes) */
int mdp_md_thermo(mdp_ctx *ctx, double out[9]);
int mdp_md_download(mdp_ctx *ctx, double *x, double *v, double *f, double *eatom); /* owned atoms; NULLs skipped */
int mdp_md_upload_x(mdp_ctx *ctx, const double *x);                             /* owned atoms [nlocal][3] */
int mdp_md_download_x_all(mdp_ctx *ctx, double *x_all); /* owned atoms then ghosts, [nlocal+nghost][3] (diagnostics) */
/* device pointers of resident arrays for zero-copy plumbing (name: "x","v","f","fp","eatom") */
void *mdp_md_ptr(mdp_ctx *ctx, const char *name);
/* statistics of the last neighbor build: out[0]=total master entries (owned; 0 if not built),
 * [1]=ghost-list entries, [2]=LJ row entries incl. padding (rebomos), [3]=REBO candidate entries, [4]=#centres,
 * [5]=#centres with at most three neighbours (one lane each), [6]=#centres in 12- and 16-lane groups, [7]=style-list
 * builds so far (rebomos) /
 * #angular atoms (aeam) */
int mdp_md_neighbor_stats(mdp_ctx *ctx, long long out[8]);
/* dynamic pruning of the tile rows in resident runs (between list builds the rows are re-filtered from the current
 * positions to the entries within window + buffer of a cluster atom; the reference walks its whole list every step,
 * pair_rebomos.cpp:490-521 -- same pairs evaluated, fewer entries tested):
 * out[0]=prunings so far, [1]=prunings that came late (an atom had moved more than half the buffer when the
 * deferred trigger was read; the analogue of LAMMPS' "dangerous builds"), [2]=1 if the kernels currently walk pruned
 * rows, [3]=buffer in units of 1e-6 Angstrom */
int mdp_md_prune_stats(mdp_ctx *ctx, long long out[4]);
/* out[0] = skin of the style's own lists in effect (rebomos: the inner skin, adaptive or MDP_INNER_SKIN; aeam: the
 * host's), [1] = cap on the inner skin, 0 = none (a candidate row outgrew the 64-bit active mask at that skin: the
 * lists were rebuilt with half of it), [2] = pruning buffer in effect (0: rows as built),
 * [3] = list builds that came late (an atom was beyond half the inner skin when the deferred trigger was read),
 * [4] = rebomos: centres that outgrew the lane-per-centre kernel (a fourth neighbour) in the last step whose count has
 * reached the host, [5] = 1 while such centres are collected on a device list and taken by the 8-lane-group kernel
 * (0: they go to the general kernel's list), [6..7] reserved */
int mdp_md_list_state(mdp_ctx *ctx, double out[8]);
/* shape of the rebomos style's own Lennard-Jones lists after the last build (host and resident mode):
 * out[0]=1 tile lists / 0 per-cluster lists (fallback), [1]=#tiles, [2]=union stride, [3]=largest union,
 * [4]=row entries incl. padding, [5]=#clusters, [6]=#tiles in the large-union launch classes,
 * [7]=style-list builds so far.  (No reference counterpart: the CPU style reads the host's list.) */
int mdp_rebomos_list_info(mdp_ctx *ctx, long long out[8]);
/* rebomos, diagnostics: which pair loops the waves of the lane-group centre kernels took in the computes run with
 * MDP_CENTRE_COUNT=1 in the environment since the last reset: out[0] = waves on the full-group path (every lane group
 * of the wave holds a centre with exactly as many neighbours as the group has lanes), out[1] = waves that hold a centre
 * and took the general loops (all of them with MDP_CENTRE_FULL=0).  reset != 0 clears both afterwards.  Waits for the
 * stream.  (No reference counterpart.) */
int mdp_rebomos_centre_paths(mdp_ctx *ctx, long long out[2], int reset);
/* ... and, over the same computes, *out = trips of the first pair loop of the waves on the full-group path that took the
 * blend of the two G(cos) polynomials (some pair of the trip had cos >= 1/2); a wave of G-lane groups makes G/2 trips.
 * The order of the candidate rows decides it (MDP_CAND_ORDER, read at each list build: 0 keeps the rows as the sweep
 * emitted them).  A count of its own: reset != 0 clears it afterwards and leaves the two above alone.  Waits for the
 * stream.  (No reference counterpart.) */
int mdp_rebomos_centre_blend_trips(mdp_ctx *ctx, long long *out, int reset);
/* how the work of the last compute was spread over the kernel classes (diagnostics of a bench line; no reference
 * counterpart -- the CPU style has one loop, pair_rebomos.cpp:358-447, pair_aeam.cpp:337-475):
 * rebomos: out[0..19] = centres per launch class at the last style-list build, class = 2 * (lane-group index: 0 one lane
 * per centre, 1..4 groups of 8 / 12 / 16 / 32 lanes) + element, + 10 for centres that reach a remote ghost;
 * [20..23] = tiles per Lennard-Jones launch class (small unions, large unions, two unused); [24] = centres the general
 * kernel's list received in the last compute whose count has reached the host (lane-group overflow); [25..28] = centres
 * with a fourth neighbour per (interior / boundary, element) list of the lane-per-centre kernel; [29] = largest tile union
 * of the small launch class, [30] = largest union.
 * aeam: out[0] = angular centres, [1] = tiles, [2] = tiles that reach no remote ghost, [30] = largest union. */
int mdp_md_class_stats(mdp_ctx *ctx, long long out[32]);

/* ---- resident mode, domain decomposition on the device ----------------------------------------------------------
 * What the reference gets from the LAMMPS host at every reneighboring -- Domain::remap, Comm::exchange,
 * Comm::borders (the REQ_GHOST list of pair_rebomos.cpp:218 presupposes them; processor grid of
 * log.rebomos-bulk.4:22) -- done per rank on the GPU: one brick of the periodic (triclinic) box per context.
 * The library packs and unpacks DEVICE buffers; the caller moves the bytes between ranks (RCCL all-to-all) and sees
 * only per-rank counts.  Sequence at a reneighboring (every rank, same step):
 *     mdp_dd_migrate_begin  -> counts of atoms leaving for each rank        [exchange counts]
 *     mdp_dd_migrate_pack   -> 8 doubles per leaver, rank-major             [exchange records]
 *     mdp_dd_migrate_end    <- arrivals; owned atoms re-ordered along a Hilbert curve over the brick
 *     mdp_dd_borders_begin  -> counts of ghost entries for each rank        [exchange counts]
 *     mdp_dd_borders_pack   -> 6 doubles per entry, rank-major              [exchange records]
 *     mdp_dd_borders_end    <- remote ghosts; then mdp_md_build_neighbors
 * and per step mdp_dd_forward_pack / _unpack (3 doubles per send-list entry).  A one-rank run needs no transport:
 * mdp_dd_reneighbor does the whole sequence.  Dimensions are periodic (as in both bundled inputs) unless
 * mdp_dd_config.nonperiodic says otherwise. */
typedef struct {
  double boxlo[3];
  double h[6];        /* xprd, yprd, zprd, yz, xz, xy  (LAMMPS Domain::h) */
  int procgrid[3];    /* bricks per dimension; rank = (ix*py + iy)*pz + iz */
  int rank;
  double cutghost;    /* ghost-shell width: the host's list cutoff, pair cutoff + skin (log.rebomos-bulk.1:43) */
  int self_remote;    /* 0.  Testing aid: 1 = periodic self-images are treated as remote ghosts that travel through the
                         transport to the rank itself (exercises every exchange with a single rank / GPU) */
  int nonperiodic[3]; /* 0 0 0 (both bundled inputs: `boundary p p p`).  1 = this dimension is not periodic (LAMMPS
                         boundary f / s / m: a slab, a free surface, a cluster): no images across it, positions are
                         not wrapped, atoms beyond the box belong to the brick at that end */
} mdp_dd_config;

int mdp_dd_setup(mdp_ctx *ctx, const mdp_dd_config *cfg); /* after mdp_md_setup (owned atoms in any order, ghosts optional) */
int mdp_dd_reneighbor(mdp_ctx *ctx);                       /* one-rank runs: remap, order, self-image ghosts, lists */
int mdp_dd_migrate_begin(mdp_ctx *ctx, int *send_counts /* [nranks] */);
int mdp_dd_migrate_pack(mdp_ctx *ctx, double *d_buf);
int mdp_dd_migrate_end(mdp_ctx *ctx, int narrive, const double *d_buf);
int mdp_dd_borders_begin(mdp_ctx *ctx, int *send_counts /* [nranks] */);
int mdp_dd_borders_pack(mdp_ctx *ctx, double *d_buf);
int mdp_dd_borders_end(mdp_ctx *ctx, const int *recv_counts /* [nranks] */, const double *d_buf);
/* out[0]=nlocal [1]=periodic self-image ghosts [2]=send-list entries [3]=remote ghosts [4]=reneighborings so far
 * [5]=atoms that left at the last one [6]=nranks [7]=rank; per-rank counts of the per-step halo (may be NULL) */
int mdp_dd_info(mdp_ctx *ctx, long long out[8], int *send_counts, int *recv_counts);
int mdp_dd_forward_pack(mdp_ctx *ctx, double *d_buf);          /* x of the send list (+ image shift) */
int mdp_dd_forward_unpack(mdp_ctx *ctx, const double *d_buf);  /* -> remote ghosts */
int mdp_dd_forward_scalar_pack(mdp_ctx *ctx, double *d_buf);   /* AEAM fp (pair_aeam.cpp:307, 946-963) */
int mdp_dd_forward_scalar_unpack(mdp_ctx *ctx, const double *d_buf);
int mdp_dd_reverse_pack(mdp_ctx *ctx, double *d_buf);          /* forces on remote ghosts (AEAM angular terms) */
int mdp_dd_reverse_unpack(mdp_ctx *ctx, const double *d_buf);  /* += onto the send-list atoms */
/* ---- the same exchanges done by the library on RCCL (csrc/comm_rccl.hip): for C++ hosts ---------------------------
 * What LAMMPS' Comm brick does over MPI for the reference (exchange / borders / forward_comm / reverse_comm; "Comm"
 * is 5.67 % of log.rebomos-bulk.4:67) as grouped ncclSend/ncclRecv between the bricks' GPUs over xGMI.  RCCL is
 * bound at run time (dlopen of librccl.so.1); MDP_ENOTIMPL if it cannot be loaded.  Rank 0 creates the id, the host
 * distributes its 128 bytes (MPI_Bcast, a file, ...), every rank calls mdp_dd_comm_init after mdp_dd_setup.  All
 * calls below are collective over the ranks and run on the context's stream; the per-step position exchange uses
 * a stream of its own between _begin and _end, so that work launched in between (mdp_md_compute_begin) overlaps it. */
int mdp_dd_comm_unique_id(void *id128);
/* Which RCCL object is bound: the name goes to buf (may be NULL).  Returns 0 for a RCCL library, 1 when MDP_RCCL_LIBRARY
 * points at the repository's TEST DOUBLE (tests/native/fake_rccl.cpp: several ranks sharing one GPU, host-staged -- a
 * rehearsal of the exchange schedule whose timings mean nothing; every report has to say so), MDP_ENOTIMPL when nothing
 * loads.  MDP_RCCL_LIBRARY=<path> binds that one object instead of librccl.so.1; nothing else is tried then. */
int mdp_dd_comm_library(char *buf, int cap);
int mdp_dd_comm_init(mdp_ctx *ctx, const void *id128);
int mdp_dd_comm_destroy(mdp_ctx *ctx);
int mdp_dd_comm_reneighbor(mdp_ctx *ctx);       /* Comm::exchange + Comm::borders + Neighbor::build */
int mdp_dd_comm_forward_begin(mdp_ctx *ctx);    /* Comm::forward_comm: x of the send list -> remote ghosts */
int mdp_dd_comm_forward_end(mdp_ctx *ctx);
int mdp_dd_comm_forward_scalar(mdp_ctx *ctx);   /* AEAM fp (pair_aeam.cpp:307) */
int mdp_dd_comm_reverse(mdp_ctx *ctx);          /* Comm::reverse_comm of f (AEAM angular terms) */
/* the two aeam exchanges of a step in one group of sends and receives on the communication stream, between
 * mdp_md_aeam_density (after mdp_md_compute_begin: three-body forces done) and mdp_md_aeam_force; work launched in
 * between (mdp_md_aeam_force_begin) overlaps them.  with_reverse = 0 leaves the ghost forces out (all ranks alike:
 * no rank has an angular centre next to a remote ghost, mdp_md_aeam_state out[3] reduced over the ranks).  _begin
 * also folds the periodic self-images' forces (mdp_md_fold_self_ghost_f). */
int mdp_dd_comm_aeam_exchange_begin(mdp_ctx *ctx, int with_reverse);
int mdp_dd_comm_aeam_exchange_end(mdp_ctx *ctx);
int mdp_dd_comm_allreduce(mdp_ctx *ctx, double *vals, int n, int op /* 0 sum, 1 max */);
/* A whole step of a multi-GPU run in two calls (what the LAMMPS host does around Pair::compute in Verlet::run:
 * initial_integrate, neighbor->decide, exchange / borders or forward_comm, force, final_integrate;
 * log.rebomos-bulk.4:22,65-67 is such a run on four ranks).  The `neigh_modify every 1 check yes` decision is collective
 * without a collective of the host's: every rank's "an owned atom moved beyond the trigger" word of a step is gathered
 * behind that step's position exchange and read -- the same value on all ranks -- at the next step.
 *   _begin: with_final = complete the half-kick a deferred step left; force_rebuild: -1 decide from the gathered word,
 *           0 never, 1 reneighbor now; *reneighbored = 1 when the call reneighbored.  Integrates, reneighbors or starts
 *           the position exchange, launches what needs no remote ghost of this step.
 *   _end:   waits for the exchange, runs the rest of the compute (aeam: fp / ghost-force exchange behind the interior
 *           pair forces when possible, the same exchanges in the blocking order otherwise), final half-kick now
 *           (defer_final = 0) or fused into the next _begin (1).
 * mdp_dd_comm_step_info: out[0] = aeam steps on the phased order, [1] = 1 if ghost forces travel, [2] = 1 if the last
 * _begin reneighbored, [3] = reneighborings so far, [4] = checks that saw an owned atom beyond half the skin,
 * [5] = overlap policy, [6] = 1 if MDP_OVERLAP_POLICY fixed it, [7] = its mean device time per step in the trial (ns).
 * Overlap policy: how a step orders its compute against its exchanges -- 0 "split" (what needs no remote ghost of this
 * step is launched behind the start of the exchange), 1 "lead" (as 0, and the compute stream waits until the RCCL kernel
 * has started), 2 "blocking" (exchange, then the whole compute: rebomos with one launch per centre class over its
 * interior and boundary halves), 3 "first" (rebomos: only the first interior kernel behind the exchange), 4 "inline"
 * (as blocking, the position exchange queued on the context's own stream: no second stream, no events).  The sends and
 * receives are the same in all of them.  The first steps of a run are a trial (blocks of 4 steps per policy, two
 * rounds; -1 in out[5] while it runs): device time per step between two events, MAX over the ranks, cheapest policy
 * kept.  MDP_OVERLAP_POLICY = split | lead | blocking | first | inline skips the trial. */
int mdp_dd_comm_step_begin(mdp_ctx *ctx, int with_final, int force_rebuild, int eflag, int vflag, int *reneighbored);
int mdp_dd_comm_step_end(mdp_ctx *ctx, int eflag, int vflag, int defer_final);
int mdp_dd_comm_step_info(mdp_ctx *ctx, long long out[8]);

/* `neigh_modify every 1 delay 0 check yes` (sample.in:17-18, log.rebomos-bulk.1:46) without a host round trip per
 * step: *moved = outcome of the check launched by the PREVIOUS call (0 right after a reneighboring), then a check of
 * the current positions is launched.  Trigger: an owned atom moved more than skin/2 - 0.1 A since the last build
 * (the margin covers the step the answer is late by); *dangerous = an atom was beyond skin/2 itself. */
int mdp_md_moved_async(mdp_ctx *ctx, int *moved, int *dangerous);
/* mdp_md_initial_integrate (with_final != 0: mdp_md_final_initial_integrate) and mdp_md_moved_async in one call and one
 * pass over the atoms: same results, the check reads the new positions while they are in registers. */
int mdp_md_integrate_check(mdp_ctx *ctx, int with_final, int *moved, int *dangerous);
/* owned atoms' "tag" / "type" / "mask" (mdp_md_set_mask) / "image" (mdp_md_set_image) in device order (the device re-orders atoms at every reneighboring); "tile_nu"
 * (diagnostics): {members of the neighbour union, Mo / first-type members} of every 32-atom tile, 2 ints per tile */
int mdp_md_download_int(mdp_ctx *ctx, const char *name, int *out);

/* ---- host mode with the integrator on the device (the plugins' `fix nve/mdp`) -----------------------------------------
 * The reference's styles run under the host's fix nve, which reads atom->f and writes atom->x / atom->v on the host
 * every step (LAMMPS Verlet::run; the reference repository itself registers a fix style from a plugin,
 * USER-BFIELD/bfieldplugin.cpp:15-29, virtuals fix_bfield.h:33-38).  With these calls a host-mode context does the two
 * half-kicks and the drift on the device: between two reneighborings of the host nothing per atom crosses the link.
 * Needs the periodic images kept by the library (mdp_set_box_host, one periodic rank).  Sequence:
 *     mdp_hnve_setup (once: dt, force->ftm2v, atom->mass[1..ntypes])
 *     at every reneighboring: mdp_set_atoms_host (+ skin / list check as before), mdp_hnve_upload_v(atom->v)
 *     per step: mdp_hnve_initial -> [compute with f == NULL: forces stay on the device] -> mdp_hnve_final
 *     mdp_hnve_download(x, v, f) before anything on the host reads them (reneighboring, thermo / dump steps)
 * mdp_hnve_initial: *moved = an owned atom has moved half the host's skin minus a margin since the last
 * mdp_set_atoms_host, as seen by the PREVIOUS call (no wait for the kernel just queued) -- the host reneighbors at its
 * next step; *dangerous = one was beyond half the skin already.  rebomos: the style's own checks (device-built lists,
 * pruned rows) ride in the same integrate kernel and are read by the NEXT compute, as in resident runs, so no call of a
 * step waits for the stream.  mdp_*_compute_host / mdp_aeam_force_host accept
 * f == NULL while the integrator is on (per-atom tallies then need f).  mdp_hnve_off: back to plain host mode. */
int mdp_hnve_setup(mdp_ctx *ctx, double dt, double ftm2v, const double *mass_per_type /* [ntypes+1], 1-based */, int ntypes);
int mdp_hnve_off(mdp_ctx *ctx);
int mdp_hnve_upload_v(mdp_ctx *ctx, const double *v /* [nlocal][3], the host's atom order */);
int mdp_hnve_initial(mdp_ctx *ctx, int *moved, int *dangerous);
int mdp_hnve_final(mdp_ctx *ctx);
int mdp_hnve_download(mdp_ctx *ctx, double *x, double *v, double *f /* [nlocal][3] each, or NULL */);

/* ---- Nose-Hoover chain thermostat on the device (LAMMPS fix nvt, thermostat only; the plugin style `fix nvt/mdp`) -----
 * Once set, the integrate calls of this context apply it: the resident ones (initial / final / final_initial /
 * integrate_check) and the host-mode ones (hnve initial / final).  Without it they run exactly the NVE code.  The chain
 * (eta, eta_dot, eta_dotdot, masses) lives on the device; the temperature is a fixed-order reduction of per-block partial
 * sums (bitwise reproducible) and the scale factor travels to the integrate kernel in device memory, so a step adds no
 * host wait.  One rank only: a brick of several ranks refuses it (and refuses to become one while it is set).
 *   setup: Tstart Tstop Tdamp, tchain (1..8) tloop drag, nf = degrees of freedom (3N - 3), boltz, mvv2e
 *   run(first, last): the ramp of the next run (target T at step n: Tstart + (n-first)/(last-first) (Tstop-Tstart));
 *                     the step counter starts at `first` and advances with every initial half; the chain masses and
 *                     the temperature are set up again at the next initial half (LAMMPS FixNH::setup)
 *   A final half deferred by the host (mdp_md_defer_final) completes inside mdp_nhc_run and mdp_nhc_off, at the target
 *   of its own step.
 *   state: out[MDP_NHC_STATE_LEN] = T, Tt, thermostat energy (ecouple), eta[8], eta_dot[9], eta_dotdot[8]
 *          (the temperature / target / energy of the last half-update)
 *   set_state: the same layout (T, Tt and the energy are ignored): seeds the chain, e.g. from an earlier run */
#define MDP_NHC_STATE_LEN 28
#define MDP_NHC_MAXCHAIN 8
typedef struct {
  double t_start, t_stop, t_period; /* temp Tstart Tstop Tdamp                                          */
  int tchain, tloop;                /* chain length (1..8), sub-steps of each half-update               */
  double drag;                      /* 0: none                                                          */
  double nf;                        /* degrees of freedom of the group (3N - 3 for all atoms)           */
  double boltz, mvv2e;              /* force->boltz, force->mvv2e                                       */
} mdp_nhc_config;
int mdp_nhc_setup(mdp_ctx *ctx, const mdp_nhc_config *cfg);
int mdp_nhc_run(mdp_ctx *ctx, long long first, long long last);
int mdp_nhc_state(mdp_ctx *ctx, double *out);
int mdp_nhc_set_state(mdp_ctx *ctx, const double *in);
int mdp_nhc_off(mdp_ctx *ctx);

/* ---- Langevin thermostat on the device (LAMMPS fix langevin without gjf / angmom / omega; the plugin style
 * `fix langevin/mdp`) -----
 * Once set, the kernel that first consumes a compute's forces adds the Langevin force of that step in registers
 * (FixLangevin::post_force): f_L = gfactor1[t] v + gfactor2[t] sqrt(T(n)) (u - 0.5) per component, with
 *   gfactor1[t] = -mass[t] / damp / ftm2v / ratio[t],  gfactor2[t] = sqrt(mass[t]) sqrt(24 boltz / damp / dt / mvv2e)
 *   / ftm2v / sqrt(ratio[t]),  T(n) = Tstart + (n - first) / (last - first) (Tstop - Tstart)
 * and v the velocities after the initial half of step n.  The kernels are those of the integrate calls: the resident
 * ones (initial / final / final_initial / integrate_check, and so the bricks step) and the host-mode ones (hnve initial
 * / final).  A final half on its own writes f + f_L back, so the next initial half uses LAMMPS' modified forces.
 * Noise: Philox4x32-10, key {seed, 0}, counter {tag, (uint32) n, (uint32) (n >> 32), phase} (phase 0: the post_force of
 * step n, 1: the setup force of the run's first step); words 0..2 give x, y, z as u = (r + 0.5) 2^-32.  The noise of
 * an atom depends on its tag and the step alone, so the trajectory does not depend on the atom order or on the number
 * of ranks.  Needs the atoms' tags.
 *   setup: see mdp_langevin_config.  zero: the mean of the random parts (over natoms) is taken out of every force.
 *          tally: the energy the thermostat has taken out (FixLangevin::compute_scalar with tally yes).  zero and tally
 *          need the whole system on one rank: a brick of several ranks refuses them (in either call order).  The
 *          Nose-Hoover chain and the Langevin thermostat refuse each other on one context.
 *   run(first, last): the ramp of the next run (steps beyond `last` hold Tstop); the step counter starts at `first`
 *          and advances with every initial half.  The next initial half applies the setup force (phase 1, at step `first`) first.
 *   tally: *out = the thermostat energy (0 without tally yes); completes a deferred final half first.
 *   A final half deferred by the host (mdp_md_defer_final) completes inside mdp_langevin_run and mdp_langevin_off.
 *   After mdp_langevin_off the forces on the device still hold the last Langevin force (LAMMPS' atom->f does too)
 *   until the next compute: a new run computes them first (Verlet::setup). */
typedef struct {
  double t_start, t_stop, t_period; /* Tstart Tstop damp (T >= 0, damp > 0)                              */
  int seed;                         /* > 0                                                               */
  int zero, tally;                  /* zero yes / tally yes                                              */
  double boltz, mvv2e;              /* force->boltz, force->mvv2e                                        */
  double ratio[16];                 /* scale: per type 1..15 (> 0; 1 when not scaled)                    */
  long long natoms;                 /* atoms in the system (zero yes divides by it)                      */
} mdp_langevin_config;
int mdp_langevin_setup(mdp_ctx *ctx, const mdp_langevin_config *cfg);
int mdp_langevin_run(mdp_ctx *ctx, long long first, long long last);
int mdp_langevin_tally(mdp_ctx *ctx, double *out);
int mdp_langevin_off(mdp_ctx *ctx);
/* Several baths on disjoint groups in one run (several `fix langevin/mdp` next to one `fix nve/mdp`): up to
 * MDP_LANGEVIN_MAXBATH thermostats, bath k on the atoms whose mask (mdp_md_set_mask / mdp_hnve_set_mask) has groupbit[k]
 * and that are inside the integrate group, each with its own configuration (natoms: the atoms of ITS group) and its own
 * tally.  All are applied in the one pass of the integrate kernels; lanes of different baths differ in the indices they
 * read, not in the code they run.
 *   baths:      replaces whatever thermostat set-up is on.  nbath == 1 is mdp_langevin_setup(cfg) followed by
 *               mdp_langevin_group(groupbit[0]): the kernels of one thermostat.  Refused (MDP_EINVAL / MDP_ESTATE, each
 *               with its cause): nbath outside 1 .. MDP_LANGEVIN_MAXBATH, a zero bit or a bit two baths share, a bath's
 *               argument errors as in mdp_langevin_setup, the Nose-Hoover chain or the minimiser on the context (in
 *               either order), zero or tally in any bath on a brick of several ranks (in either call order), and atoms
 *               of the current mask that are in more than one bath -- LAMMPS would add both forces on such an atom, the
 *               device refuses it and says how many there are.  That count is taken once per mdp_langevin_baths and per
 *               mask upload, never in a step.  An integrate call with several baths and no mask fails with MDP_ESTATE,
 *               and so does mdp_langevin_group while several baths are on.
 *   run / off:  apply to all baths: one first / last, one step counter, one setup force.
 *   tally:      the sum over the baths, in bath order (what `ecouple` adds up).
 *   tally_bath: *out = the energy bath k has taken out (0 without tally yes); with one thermostat on, k = 0. */
#define MDP_LANGEVIN_MAXBATH 4
int mdp_langevin_baths(mdp_ctx *ctx, int nbath, const mdp_langevin_config *cfg, const int *groupbit);
int mdp_langevin_tally_bath(mdp_ctx *ctx, int bath, double *out);

/* ---- Constant-flux heat sources on groups (LAMMPS fix heat with a constant eflux and no region; the plugin style
 * `fix heat/mdp`) -----
 * Up to MDP_HEAT_MAXSRC sources, source k on the atoms whose mask (mdp_md_set_mask / mdp_hnve_set_mask) has groupbit[k].
 * Every final half that completes step n -- mdp_md_final_integrate, mdp_hnve_final, a deferred final half completed by a
 * thermo / download / state read, the final half of mdp_md_final_initial_integrate -- is followed on the stream by the
 * heat pass of step n for the sources with n % nevery == 0 (FixHeat::end_of_step):
 *     heat   = eflux nevery dt ftm2v,   ke = (0.5 sum m v.v mvv2e) ftm2v,   vcm = sum m v / M      (sums over the group)
 *     escale = (ke + heat - 0.5 vcm.vcm M) / (ke - 0.5 vcm.vcm M),   scale = sqrt(escale),   v = scale v - (scale - 1) vcm
 * so the group keeps its momentum and its kinetic energy about its centre of mass changes by eflux nevery dt.  Three
 * launches: per-block partial sums in fixed slots, one workgroup that adds them in a fixed order and leaves scale and
 * (scale - 1) vcm in device memory, and the pass that rescales.  No float atomics, no host wait: a run is bitwise
 * reproducible, and the same whether or not the host defers final halves -- with sources on the final and the initial
 * half are never fused into one kernel.  dt and ftm2v are the context's own; M is summed once per set-up and mask upload.
 *   setup:  replaces the sources that are on.  A final half pending at the call completes first, without heat.  Refused
 *           (MDP_EINVAL / MDP_ESTATE, each with its cause): nsrc outside 1 .. MDP_HEAT_MAXSRC, a zero bit or a bit two
 *           sources share, nevery < 1, a non-finite eflux, no mask for the current atoms, a source without atoms, atoms
 *           in two sources and source atoms outside the integrate group (both with their count, taken on the device once
 *           per set-up and per mask upload), a thermostat (mdp_nhc_setup, mdp_langevin_*) or the minimiser on the
 *           context and a brick of several ranks -- those calls in turn refuse while sources are on.
 *   run:    the step counter of the run that follows = first; it advances with every initial half, and a final half
 *           before the first initial half (it belongs to the run before) gets no pass: step `first` is never heated.
 *   state:  blocking; completes a deferred final half first.  out[0] scale of source src's last application (1 before
 *           the first), [1..4) vcm, [4] the kinetic energy about the centre of mass before it (times ftm2v, as ke above),
 *           [5] M, [6] applications so far, [7] the step of a latched error or -1.
 *   errors: escale < 0 or a denominator that is not positive latches (step, source) on the device; this and every later
 *           application leave v alone.  The next call that waits for the stream anyway (mdp_md_thermo, mdp_md_download,
 *           mdp_hnve_download, mdp_heat_state, mdp_sync) fails with MDP_ESTATE "fix heat kinetic energy went negative
 *           (source k, step n)", until mdp_heat_off. */
#define MDP_HEAT_MAXSRC 4
#define MDP_HEAT_STATE_LEN 8
typedef struct {
  double eflux;  /* energy / time, either sign */
  int nevery;
  double mvv2e;
} mdp_heat_config;
int mdp_heat_setup(mdp_ctx *ctx, int nsrc, const mdp_heat_config *cfg, const int *groupbit);
int mdp_heat_run(mdp_ctx *ctx, long long first);
int mdp_heat_state(mdp_ctx *ctx, int src, double *out /* MDP_HEAT_STATE_LEN */);
int mdp_heat_off(mdp_ctx *ctx);

/* ---- Indenters: spheres, cylinders and planes that push on the atoms (LAMMPS fix indent with `units box` and a centre
 * that moves at a constant velocity; the plugin style `fix indent/mdp`) -----
 * Up to MDP_INDENT_MAX indenters, indenter k on the owned atoms whose mask has groupbit[k]; a bit of 0 means every owned
 * atom and needs no mask.  Indenters may share atoms: their forces add.  For the forces of step n the centre is
 *     ctr = c + vel (n - first) dt                                   (LAMMPS' vdisplace(c, vel); dt is the context's own)
 * and an atom at x, with D = x - ctr through Domain::minimum_image of the context's box (mdp_dd_setup / mdp_set_box_host:
 * one wrap per periodic dimension, z then y then x, a wrap in z carrying (xz, yz) and one in y carrying xy), feels what
 * follows.  A brick's periodicity is that of mdp_dd_config; the box of mdp_set_box_host carries no boundary flags and is
 * taken to be periodic in all three dimensions (what that call is for: one periodic rank) -- a host whose box is not must
 * not set indenters on a host-linked context, and the plugin's fix refuses such a box.
 *     sphere, cylinder (D without its component along dim):  r = |D|,  dr = r - R (side out) or R - r (side in)
 *     plane:  dr = x[dim] - c[dim] (lo) or c[dim] - x[dim] (hi); no minimum image, as in LAMMPS
 *     dr < 0:  a force of magnitude K dr^2 out of the indenter's body (along D / r for side out, against it for side in,
 *              along +dim for lo and -dim for hi); the indenter's energy gains -K/3 dr^3, the force on the indenter
 *              minus the atom's force.  r == 0: no force (LAMMPS divides by zero there), the energy is counted.
 * The pass is two launches: one lane per owned atom adds the force into f and the blocks leave per-indenter sums in
 * fixed slots; one workgroup adds the slots in a fixed order and leaves the state in device memory.  No float atomics and
 * no host wait: a run is bitwise reproducible, and the same whether or not the host defers final halves.
 * Every kick of v by f begins with the pass unless the forces the context holds have had theirs already.  That flag is
 * cleared behind every initial half (a compute follows and overwrites f) and by _setup / _run, which take the forces of
 * the context at the call to be the pair style's alone -- true of what Verlet::setup has just computed; a host that calls
 * either in mid-run computes the forces again before its next kick.  The step of the current forces is `first` plus the
 * initial halves since _run.  The minimiser does not run the pass.
 *   setup:  replaces the indenters that are on.  A final half pending at the call completes first, without indenters.
 *           Refused (MDP_EINVAL / MDP_ESTATE, each with its cause): n outside 1 .. MDP_INDENT_MAX, K or R negative or not
 *           finite, a centre or velocity that is not finite, a shape, dim or side out of range, a cylinder with a velocity
 *           along its axis, a group bit with no mask for the current atoms, no box on the context, the minimiser, the
 *           Nose-Hoover chain or heat sources on the context and a brick of several ranks -- those calls in turn refuse
 *           while indenters are on.  Langevin thermostats are welcome.
 *   run:    a final half pending at the call completes first, with the pass of its step if that is still due; then the
 *           centre starts again at c: the forces the context holds count as those of step `first`, without a pass.
 *   state:  blocking; completes a deferred final half, and runs the pass if the current forces have not had it (the
 *           state of step `first` before any kick).  out[0] energy, [1..4) force on the indenter, [4] atoms in contact,
 *           [5] the step these belong to, [6..9) the centre at that step, [9] passes since setup.
 *   off:    a pending final half completes first, with its pass; frees what was held. */
#define MDP_INDENT_MAX 4
#define MDP_INDENT_STATE_LEN 10
enum { MDP_INDENT_SPHERE = 0, MDP_INDENT_CYLINDER = 1, MDP_INDENT_PLANE = 2 };
typedef struct {
  int shape;     /* MDP_INDENT_SPHERE, _CYLINDER, _PLANE */
  int dim;       /* 0, 1, 2: the cylinder's axis, the plane's normal; a sphere ignores it */
  int side;      /* sphere, cylinder: 0 out, 1 in; plane: 0 lo, 1 hi */
  double k;      /* force / length^2 */
  double c[3];   /* the centre at step `first`; a cylinder uses the two components across dim, a plane c[dim] */
  double r;
  double vel[3]; /* length / time */
} mdp_indent_config;
int mdp_indent_setup(mdp_ctx *ctx, int n, const mdp_indent_config *cfg, const int *groupbit);
int mdp_indent_run(mdp_ctx *ctx, long long first);
int mdp_indent_state(mdp_ctx *ctx, int k, double *out /* MDP_INDENT_STATE_LEN */);
int mdp_indent_off(mdp_ctx *ctx);

/* ---- Tether springs on a group's centre of mass (LAMMPS fix spring tether, with the constant-velocity tether point of
 * fix smd; the plugin style `fix spring/mdp`) -----
 * Up to MDP_SPRING_MAX springs, spring k on the owned atoms whose mask has groupbit[k]; a bit of 0 means every owned atom
 * and needs no mask.  Springs may share atoms: their forces add.  For the forces of step n the tether point is
 *     p = c + vel (n - first) dt                                                     (dt is the context's own)
 * and a dimension d with use[d] == 0 (LAMMPS' NULL) takes no part: its component of d below is 0, its vel is ignored.
 * With xu_i = x_i + h . image_i over the atoms of the group (the image flags of mdp_md_set_image, the box of mdp_dd_setup):
 *     M = sum m_i,  xcm = (sum m_i xu_i) / M,  d = xcm - p,  r = max(|d|, 1e-10),  dr = r - R0
 *     F = K d dr / r,  E = K dr^2 / 2,  f_i -= (F / M) m_i,  ftotal = (-Fx, -Fy, -Fz, sign(dr) |F|)
 * The pass is three launches: per block and spring the sums in fixed slots; one workgroup that adds the slots in a fixed
 * order, forms the above and leaves the state and F / M in device memory; one lane per owned atom that takes its share off
 * f, spring after spring.  No float atomics and no host wait: a run is bitwise reproducible, and the same whether or not
 * the host defers final halves.  M is summed in two parts that add exactly (up to 2^22 atoms with masses in [1, 2048)):
 * the state's M is the correctly rounded sum of the masses, whatever order the device holds the atoms in.
 * Every kick of v by f begins with the pass unless the forces the context holds have had theirs already -- behind the
 * indenters' pass when both are on; that order is fixed and only affects the rounding of f.  The flag is cleared behind
 * every initial half and by _setup / _run, under the rules of mdp_indent_* (above), call for call.
 *   setup:  replaces the springs that are on.  A final half pending at the call completes first, without springs.
 *           Refused (MDP_EINVAL / MDP_ESTATE, each with its cause, before anything on the context changes): n outside
 *           1 .. MDP_SPRING_MAX, K or R0 negative or not finite, a tether point or velocity that is not finite, use all
 *           zero, a group bit with no mask for the current atoms, no image flags (mdp_md_set_image), a host-linked
 *           context (its host keeps the image flags), a brick of several ranks, the minimiser, the Nose-Hoover chain or
 *           heat sources on the context -- those calls in turn refuse while springs are on -- and a spring whose group
 *           holds no atom or no mass.  Langevin thermostats and indenters are welcome.
 *   run:    a final half pending at the call completes first, with the pass of its step if that is still due; then the
 *           tether point starts again at c: the forces the context holds count as those of step `first`, without a pass.
 *   state:  blocking; completes a deferred final half, and runs the pass if the current forces have not had it.
 *           out[0] E, [1..4) ftotal x, y, z, [4] sign(dr) |F|, [5] the step these belong to, [6..9) xcm (unwrapped),
 *           [9..12) the tether point (0 in a dimension that takes no part), [12] M, [13] atoms, [14] passes since setup,
 *           [15] 0.
 *   off:    a pending final half completes first, with its pass; frees what was held. */
#define MDP_SPRING_MAX 4
#define MDP_SPRING_STATE_LEN 16
typedef struct {
  double k, r0;  /* force / length, length */
  double c[3];   /* the tether point at step `first` */
  int use[3];    /* 0: the dimension takes no part (LAMMPS' NULL) */
  double vel[3]; /* length / time */
} mdp_spring_config;
int mdp_spring_setup(mdp_ctx *ctx, int n, const mdp_spring_config *cfg, const int *groupbit);
int mdp_spring_run(mdp_ctx *ctx, long long first);
int mdp_spring_state(mdp_ctx *ctx, int k, double *out /* MDP_SPRING_STATE_LEN */);
int mdp_spring_off(mdp_ctx *ctx);

/* ---- Prescribed forces on groups (LAMMPS fix setforce, fix addforce and fix aveforce with constant values; the plugin
 * styles `fix setforce/mdp`, `fix addforce/mdp`, `fix aveforce/mdp`) -----
 * Up to MDP_GFORCE_MAX slots, slot k on the owned atoms whose mask has groupbit[k]; a bit of 0 means every owned atom and
 * needs no mask.  The slots act in order k = 0 .. n - 1 on one atom's force, as LAMMPS' fixes do in the order of their
 * definition.  With g the atom's force as the slots before k left it, f the slot's values and use[d] == 0 LAMMPS' NULL:
 *     SET:  F_k += g;                                  then g[d] = f[d] where use[d]
 *     ADD:  F_k += g,  E_k -= f . xu  (xu = x + h . image);  then g += f
 *     AVE:  F_k += g,  N_k += 1;  then g[d] = F_k[d] / N_k + f[d] where use[d], the sums over the whole group
 * F_k is LAMMPS' f_ID[1..3] of all three styles (the group's total force before the fix acted), E_k the f_ID of addforce.
 * Only an AVE slot needs a sum over the group before an atom's later force is known, so a slot must not share atoms with
 * an AVE slot in front of it: then an atom's slots are local up to at most one AVE, the last of them, and the pass walks
 * them in one go on a running force in registers.  Every other sharing is allowed.
 * The pass: per block and slot the sums of F_k and E_k and the atom counts in fixed slots; one workgroup that adds the
 * slots in a fixed order and leaves the state and, for AVE slots, the value to write in device memory; one lane per owned
 * atom that writes the result into f.  With no AVE slot on the first kernel writes f itself and the pass is two launches.
 * No float atomics and no host wait: a run is bitwise reproducible, and the same whether or not the host defers final
 * halves.  An atom in no slot is neither read nor written.
 * Every kick of v by f begins with the pass unless the forces the context holds have had theirs already -- behind the
 * indenters' and the springs' passes when those are on, and in front of the Langevin force, which the kick itself adds:
 * a bath atom under SET or AVE still feels its bath.  The flag is cleared behind every initial half and by _setup / _run,
 * under the rules of mdp_indent_* (above), call for call.
 *   setup:  replaces the slots that are on.  A final half pending at the call completes first, without them.
 *           Refused (MDP_EINVAL / MDP_ESTATE, each with its cause, before anything on the context changes): n outside
 *           1 .. MDP_GFORCE_MAX, an unknown kind, a value that is not finite, an ADD slot with a dimension off, a group bit
 *           with no mask for the current atoms, a slot whose group holds no atom, a slot that shares atoms with an AVE
 *           slot in front of it (the message gives the count and both slots), an ADD slot without image flags
 *           (mdp_md_set_image) or on a host-linked context (its host keeps the image flags; SET and AVE do run there), a
 *           brick of several ranks, the minimiser, the Nose-Hoover chain or heat sources on the context -- those calls in
 *           turn refuse while the stage is on.  Langevin thermostats, indenters and springs are welcome.  A mask upload
 *           while the stage is on counts the sharing again and fails with the same message (the mask stays; the next pass
 *           refuses too), as a mask upload does under heat sources.
 *   run:    a final half pending at the call completes first, with the pass of its step if that is still due; the forces
 *           the context holds then count as those of step `first`, without a pass.
 *   state:  blocking; completes a deferred final half, and runs the pass if the current forces have not had it.
 *           out[0] E_k (0 unless ADD), [1..4) F_k, [4] the atoms of the slot's group, [5] the step these belong to,
 *           [6..9) the value written or added per dimension (AVE: the average plus f; 0 where not used), [9] passes
 *           since setup.
 *   off:    a pending final half completes first, with its pass; frees what was held. */
#define MDP_GFORCE_MAX 4
#define MDP_GFORCE_STATE_LEN 10
enum { MDP_GFORCE_SET = 0, MDP_GFORCE_ADD = 1, MDP_GFORCE_AVE = 2 };
typedef struct {
  int kind;      /* MDP_GFORCE_SET, _ADD, _AVE */
  int use[3];    /* 0: the dimension is left alone (LAMMPS' NULL); an ADD slot has all three on */
  double f[3];   /* force */
} mdp_gforce_config;
int mdp_gforce_setup(mdp_ctx *ctx, int n, const mdp_gforce_config *cfg, const int *groupbit);
int mdp_gforce_run(mdp_ctx *ctx, long long first);
int mdp_gforce_state(mdp_ctx *ctx, int k, double *out /* MDP_GFORCE_STATE_LEN */);
int mdp_gforce_off(mdp_ctx *ctx);

/* ---- FIRE minimiser on the device (LAMMPS min_style fire, FIRE 2.0 with the eulerimplicit integrator and LAMMPS' defaults)
 * For a resident context on one rank, after mdp_md_setup + mdp_dd_setup (one brick) + mdp_dd_reneighbor.  An iteration
 * is two small launches next to the force compute: per-block partial sums of v.f, v.v, f.f and the largest |v_c| in
 * fixed slots, then one workgroup that adds them in a fixed order, takes the decisions of the iteration (and the stop
 * tests of the one before) and leaves dtv, the mixing factors and the flags in device memory for the advance kernel.
 * The host never waits for them: it polls a pinned stop word and may queue an iteration or two too many, which change
 * nothing -- once the stop code is latched a queued advance kernel leaves x, v and the counters alone.
 *   setup:   zeroes v, computes the initial energy and force norm.  The starting time step is the context's dt, which
 *            is not changed.  Refused on a brick of several ranks and with a thermostat on the context (and the
 *            thermostats and mdp_dd_setup with several ranks are refused while it is on); a deferred final half is
 *            completed first.  ftol: sqrt(sum f.f) < ftol; etol (only when > 0): |E - Eprev| < etol (|E| + |Eprev| +
 *            1e-8) / 2, tested only more than delaystep iterations after the last P <= 0.
 *   iterate: queues up to n iterations (sums, control, advance, a reneighbouring when the device's displacement check
 *            asked for one, the compute: force-only unless etol > 0); *stop = the stop code the host has seen so far.
 *   state:   blocking.  out[MDP_FIRE_STATE_LEN] = [0] stop code [1] iterations [2] force evaluations [3] dt [4] alpha
 *            [5] sqrt(sum f.f) of the current forces [6] initial [7] previous [8] last energy (with etol == 0 the previous
 *            one is not known and repeats the last, which one energy compute gives; the forces are left as they
 *            were) [9] reneighbourings since setup [10] dtv [11] dtv of the iteration before [12] s1 [13] s2 [14] mixed
 *            (P > 0) [15] zeroed (P <= 0) [16] iteration of the last P <= 0 [17] number of P <= 0 [18] P [19] initial
 *            sqrt(sum f.f) [20] displacement checks that found an atom beyond half the skin already (a late reneighbouring)
 *   off:     back to the integrate kernels with the context's dt; v stays as the minimiser left it (zero it, or draw
 *            new velocities, before a run). */
enum { MDP_FIRE_RUNNING = 0, MDP_FIRE_FTOL = 1, MDP_FIRE_ETOL = 2, MDP_FIRE_MAXITER = 3, MDP_FIRE_MAXEVAL = 4 };
#define MDP_FIRE_STATE_LEN 21
typedef struct {
  double etol, ftol;
  long long maxiter, maxeval;
  double dmax;                  /* 0.1  */
  double tmax, tmin;            /* 10, 0.02: dt stays in [tmin, tmax] x the starting dt */
  int delaystep;                /* 20   */
  double dtgrow, dtshrink;      /* 1.1, 0.5   */
  double alpha0, alphashrink;   /* 0.25, 0.99 */
  int halfstepback, initialdelay; /* yes, yes */
} mdp_fire_config;
int mdp_fire_setup(mdp_ctx *ctx, const mdp_fire_config *cfg);
int mdp_fire_iterate(mdp_ctx *ctx, long long n, int *stop);
int mdp_fire_state(mdp_ctx *ctx, double *out);
int mdp_fire_off(mdp_ctx *ctx);

/* ---- groups of atoms (LAMMPS `fix ID GROUP ...`: the per-atom 32-bit atom->mask and a group's bit) --------------------
 * The device keeps the owned atoms' mask and the integrate calls honour two group bits.
 *   mdp_md_set_mask:     resident mode.  mask[nlocal] in the CURRENT device order (the order of mdp_md_download and
 *                        mdp_md_download_int("tag"); right after mdp_md_setup the order of the arrays handed to it).  From
 *                        then on the mask follows its atom through every reneighboring and migration (the migration record
 *                        stays 8 doubles: type and mask share one of them); mdp_md_download_int("mask") reads it back.
 *                        NULL withdraws the mask; so does mdp_md_setup.  Every rank of a brick run sets one, or none does.
 *   mdp_hnve_set_mask:   host-linked mode.  mask[nlocal] in the host's order, at every reneighboring after
 *                        mdp_set_atoms_host (next to mdp_hnve_upload_v); NULL withdraws it.
 *   mdp_integrate_group: groupbit != 0: only atoms with mask & groupbit get the half-kicks, the drift, the Nose-Hoover
 *                        scale and the FIRE advance; every other atom keeps x and v bit for bit (LAMMPS fix nve on a
 *                        group; for the minimiser, fix setforce 0 0 0 on the complement: held atoms are left out of its
 *                        sums and its force norm, and mdp_fire_setup leaves their velocities alone).  The Nose-Hoover
 *                        temperature is that of the group; nf of mdp_nhc_config is the caller's (3 N_group - 3).
 *                        0 (default): every atom, through exactly the kernels of a context without groups.
 *   mdp_langevin_group:  groupbit != 0: only atoms with mask & groupbit (and inside the integrate group) receive the
 *                        Langevin force; `zero` and `tally` run over them, natoms of mdp_langevin_config is their count.
 * Both group calls are refused (MDP_ESTATE) while the minimiser is on.  An integrate call with a non-zero group and no
 * mask for the current atoms fails with MDP_ESTATE. */
int mdp_md_set_mask(mdp_ctx *ctx, const int *mask);
int mdp_hnve_set_mask(mdp_ctx *ctx, const int *mask);
int mdp_integrate_group(mdp_ctx *ctx, int groupbit);
int mdp_langevin_group(mdp_ctx *ctx, int groupbit);

/* ---- image flags and the mean-squared displacement (LAMMPS atom->image, compute msd) ----------------------------------
 * The device keeps the owned atoms' image flag, LAMMPS' 32-bit imageint (ix + 512) | (iy + 512) << 10 | (iz + 512) << 20.
 *   mdp_md_set_image:   resident mode.  image[nlocal] in the CURRENT device order, as mdp_md_set_mask takes the mask.  From
 *                       then on every reneighboring adds the box vectors its remap takes off an atom to the atom's flag
 *                       (periodic dimensions only; a field wraps modulo 1024 as LAMMPS' does), and the flag follows its atom
 *                       through the re-ordering and the migration.  The migration record stays 8 doubles: with an image,
 *                       r[6] = type + 64 mask + 2^38 (iz + 512) and r[7] = tag + 2^31 ((ix + 512) | (iy + 512) << 10), both
 *                       exact in a double; without one the record is what it always was.  The minimiser reneighbours through
 *                       the same remap and keeps the flag too.  mdp_md_download_int("image") reads it back.  NULL withdraws
 *                       it; so does mdp_md_setup.  Every rank of a brick run sets one, or none does.
 *   mdp_md_download_unwrapped: xu[nlocal][3] = x + h . image of the owned atoms in device order, with the triclinic box of
 *                       mdp_dd_setup: xu_x = x + h0 ix + h5 iy + h4 iz, xu_y = y + h1 iy + h3 iz, xu_z = z + h2 iz.
 *   mdp_msd_setup:      starts a measurement.  x0_by_tag[ntag][3]: the unwrapped origin of the atom with tag t at [t - 1], for
 *                       ALL atoms of the system on every rank (24 bytes per atom; an atom that migrates finds its origin on its
 *                       new rank).  NULL: the current unwrapped positions of the owned atoms -- one rank only (ntag = nlocal);
 *                       refused (MDP_ESTATE) on a brick of several ranks, where an arrival's origin would be unknown.
 *                       groupbit != 0: the atoms with mask & groupbit only; needs a mask (MDP_ESTATE without one).
 *   mdp_msd_sums:       blocking.  out = this rank's sums over the group's owned atoms of dx^2, dy^2, dz^2, 1, m xu_x, m xu_y,
 *                       m xu_z, m, with d = xu - x0[tag - 1] - shift (shift NULL: 0).  The caller divides by the count, and on
 *                       several ranks sums over the ranks first.  LAMMPS' `com yes` is two calls: the mass sums give the
 *                       centre of mass cm(t), then shift = cm(t) - cm(0).  Fixed-order sums: two reads of one state agree
 *                       bit for bit.  MDP_EINVAL if an owned atom of the group has a tag outside 1 .. ntag.
 *   mdp_msd_info:       out = {a measurement is on, its ntag, its groupbit, its serial}.  The serial is unique in the process
 *                       (every mdp_msd_setup takes the next number, over all contexts): two users of one context tell by
 *                       it whether the origins the context holds are still theirs.
 *   mdp_msd_off:        releases the origins.
 * All but mdp_md_set_image are refused (MDP_ESTATE) without mdp_dd_setup and without an image. */
int mdp_md_set_image(mdp_ctx *ctx, const int *image);
int mdp_md_download_unwrapped(mdp_ctx *ctx, double *xu);
int mdp_msd_setup(mdp_ctx *ctx, int ntag, const double *x0_by_tag, int groupbit);
int mdp_msd_sums(mdp_ctx *ctx, const double *shift, double out[8]);
int mdp_msd_info(mdp_ctx *ctx, long long out[4]);
int mdp_msd_off(mdp_ctx *ctx);

/* ---- pair-distance histograms: g(r) and coordination numbers (LAMMPS compute rdf), in integers ---------------------------
 * For a resident context with mdp_dd_setup (MDP_ESTATE otherwise).  Nothing of a run is changed by a read: the binning is
 * the measurement's own.
 *   mdp_rdf_setup:   starts a measurement of npair columns (1 .. MDP_RDF_MAXPAIR) of nbin bins over 0 <= r < cutoff.  Column m
 *                    counts the pairs with type(i) in ilo[m] .. ihi[m] and type(j) in jlo[m] .. jhi[m] (LAMMPS types
 *                    1 .. ntypes, inclusive).  member_by_tag[ntag]: non-zero at [t - 1] if the atom with tag t belongs to
 *                    the group, for ALL atoms of the system on every rank (a ghost is looked up by its tag; an atom that
 *                    migrates keeps its membership); NULL: every atom.  A second call replaces the first.
 *                    MDP_EINVAL: nbin < 1, npair outside 1 .. MDP_RDF_MAXPAIR, a type outside 1 .. ntypes, lo > hi,
 *                    cutoff <= 0, nbin * npair > MDP_RDF_MAXCOUNTERS (the workgroup's histogram in LDS: 32 KB of 32-bit
 *                    counters), and cutoff + skin > the cutghost of mdp_dd_setup: the ghost shell is as of the last
 *                    reneighbouring and atoms have since moved up to half a skin each, so only the pairs within
 *                    cutghost - skin are guaranteed present.
 *   mdp_rdf_counts:  blocking.  hist[m][b] = this rank's number of ordered pairs (i owned, j owned or ghost, j != i as an
 *                    array entry -- a periodic image of an atom is a separate j, the atom's own image included, as LAMMPS'
 *                    ghost atoms are) of members with the types of column m and b = (int) (r nbin / cutoff) < nbin,
 *                    r = sqrt(dx^2 + dy^2 + dz^2) in double from the current positions.  icount[m], jcount[m], dup[m]: this
 *                    rank's owned members whose type lies in the i range, the j range, both.  The caller sums the four arrays
 *                    over the ranks and normalises.  All integers: two reads of one state agree exactly, and the sum over
 *                    the bricks equals the one-brick histogram.  MDP_ESTATE without a setup; MDP_EINVAL if an owned or ghost
 *                    atom has a tag outside 1 .. ntag of the member table.
 *                    Types: a resident context has 1 .. 15 atom types (mdp_md_setup refuses more), which is what the 4-bit
 *                    type code of the cell-ordered records and the 16 x 16 table of column masks hold.
 *   mdp_rdf_info:    out = {a measurement is on, its nbin, its npair, its serial}; the serial is unique in the process, as
 *                    that of mdp_msd_info: two users of one context tell by it whether the setup is still theirs.
 *   mdp_rdf_off:     releases the tables and the buffers of the binning. */
#define MDP_RDF_MAXPAIR 32
#define MDP_RDF_MAXCOUNTERS 8192
int mdp_rdf_setup(mdp_ctx *ctx, int nbin, double cutoff, int npair, const int *ilo, const int *ihi, const int *jlo,
                  const int *jhi, int ntag, const unsigned char *member_by_tag);
int mdp_rdf_counts(mdp_ctx *ctx, long long *hist, long long *icount, long long *jcount, long long *dup);
int mdp_rdf_info(mdp_ctx *ctx, long long out[4]);
int mdp_rdf_off(mdp_ctx *ctx);

/* ---- bond-angle histograms: the angular distribution function (LAMMPS compute adf), in integers ------------------------------
 * For a resident context with mdp_dd_setup (MDP_ESTATE otherwise), next to its one rdf measurement.  Nothing of a run is changed
 * by a read: the binning is the measurement's own (the same stage as mdp_rdf_counts').
 *   mdp_adf_setup:   starts a measurement of ntriple triples (1 .. MDP_ADF_MAXTRIPLE) of nbin bins.  Triple m has the centre
 *                    types ilo[m] .. ihi[m], the j types jlo[m] .. jhi[m] inside the shell rjin[m] <= r < rjout[m] and the k
 *                    types klo[m] .. khi[m] inside rkin[m] <= r < rkout[m] (LAMMPS types 1 .. ntypes, inclusive).  ordinate:
 *                    MDP_ADF_DEGREE, _RADIAN or _COSINE.  member_by_tag as in mdp_rdf_setup.  A second call replaces the first.
 *                    MDP_EINVAL: nbin < 1, an ordinate outside the three, ntriple outside 1 .. MDP_ADF_MAXTRIPLE (a neighbour's
 *                    j- and k-qualifications are 32-bit masks), a type outside 1 .. ntypes, lo > hi, a radius < 0, inner >=
 *                    outer, nbin * ntriple > MDP_ADF_MAXCOUNTERS (the workgroup's histogram in LDS), a member table with
 *                    ntag < 1, and an outer radius + skin > the cutghost of mdp_dd_setup, for the reason given at mdp_rdf_setup.
 *   mdp_adf_counts:  blocking.  A centre i of triple m is an owned member whose type lies in the i range; icount[m] counts
 *                    them on this rank, with or without neighbours.  A neighbour is any other array entry, owned or ghost (a
 *                    periodic image of an atom is a separate entry, the centre's own image included, as in mdp_rdf_counts).
 *                    It is a j-neighbour of triple m when it is a member, its type lies in the j range and rjin^2 <= rsq <
 *                    rjout^2, and a k-neighbour by the same rule with the k range and radii.  Every ORDERED pair (j, k), j != k
 *                    as array entries, counts once -- a triple whose j and k selections coincide counts each angle twice, as
 *                    LAMMPS does -- with c = clamp(d_ij . d_ik / (r_ij r_ik), -1, 1), the ordinate u = acos(c) 180 / pi,
 *                    acos(c) or c over [lo, hi] = [0, 180], [0, pi] or [-1, 1], and the bin b = (int) ((u - lo) nbin /
 *                    (hi - lo)), b >= nbin going into bin nbin - 1 (180 degrees and c = 1 land in the last bin).  All in double.
 *                    hist[m][b] is this rank's number of them; the caller sums hist and icount over the ranks and normalises.
 *                    All integers: two reads of one state agree exactly.  MDP_ESTATE without a setup; MDP_EINVAL if an owned
 *                    or ghost atom has a tag outside the member table, if the largest outer radius has outgrown the ghost
 *                    shell, and if a centre has more members inside the largest outer radius than MDP_ADF_MAXNEIGH (the
 *                    short list a wave keeps in LDS): the message names the number of such centres and the cap, and no
 *                    histogram is handed back -- no centre is ever truncated.  The cost is quadratic in the neighbours.
 *   mdp_adf_info:    out = {a measurement is on, its nbin, its ntriple, its serial}; the serial as that of mdp_rdf_info.
 *   mdp_adf_off:     releases the tables and the buffers of the binning. */
#define MDP_ADF_MAXTRIPLE 32
#define MDP_ADF_MAXCOUNTERS 8192
#define MDP_ADF_MAXNEIGH 128
#define MDP_ADF_DEGREE 0
#define MDP_ADF_RADIAN 1
#define MDP_ADF_COSINE 2
int mdp_adf_setup(mdp_ctx *ctx, int nbin, int ordinate, int ntriple, const int *ilo, const int *ihi, const int *jlo,
                  const int *jhi, const int *klo, const int *khi, const double *rjin, const double *rjout, const double *rkin,
                  const double *rkout, int ntag, const unsigned char *member_by_tag);
int mdp_adf_counts(mdp_ctx *ctx, long long *hist, long long *icount);
int mdp_adf_info(mdp_ctx *ctx, long long out[4]);
int mdp_adf_off(mdp_ctx *ctx);

/* ---- per-atom structure: coordination numbers and the centro-symmetry parameter (LAMMPS compute coord/atom cutoff and
 * compute centro/atom without axes) ----------------------------------------------------------------------------------------
 * For a resident context with mdp_dd_setup (MDP_ESTATE otherwise), one measurement of each kind next to the others.  Nothing of
 * a run is changed by a read: the binning is the measurement's own (the stage of mdp_rdf_counts, without a member table:
 * partners of any group count).  A centre is an owned atom with mask & groupbit (mdp_md_set_mask; groupbit 0: every owned
 * atom); a partner is any other array entry, owned or ghost (a periodic image is a separate entry, the centre's own included),
 * with rsq = dx^2 + dy^2 + dz^2 < cutoff^2 in double from the current positions.
 *   mdp_coord_setup:   ncol columns (1 .. MDP_COORD_MAXCOL: a partner's columns are one mask word); column m counts the
 *                      partners whose type lies in jlo[m] .. jhi[m] (LAMMPS types 1 .. ntypes, inclusive).  A second call
 *                      replaces the first.  MDP_EINVAL: ncol outside 1 .. MDP_COORD_MAXCOL, a type outside 1 .. ntypes,
 *                      lo > hi, cutoff <= 0, cutoff + skin > the cutghost of mdp_dd_setup (see mdp_rdf_setup).
 *   mdp_coord_read:    blocking.  tag[i] and values[i][0 .. ncol) of this rank's nlocal owned atoms in the context's owned
 *                      order (that of mdp_md_download): the counts as doubles, 0 in every column for an atom outside the
 *                      group.  Integer counts: two reads of one state agree exactly.  MDP_ESTATE without a setup, or with a
 *                      group bit and no mask that covers the current atoms; MDP_EINVAL if the cutoff has outgrown the shell.
 *   mdp_coord_info:    out = {a measurement is on, its ncol, its groupbit, its serial}; the serial as that of mdp_rdf_info.
 *   mdp_centro_setup:  nnn even, 2 .. MDP_CENTRO_MAXN (12 for fcc, 8 for bcc); cutoff <= 0 stands for the ghost shell's limit,
 *                      cutghost - skin, as it is at the setup.  MDP_EINVAL: nnn odd or outside the range, cutoff beyond the
 *                      limit.  A second call replaces the first.
 *   mdp_centro_read:   blocking.  tag[i] and values[i] as above.  Of the partners of a centre the nnn nearest are taken --
 *                      ordered by (rsq, place in the binning's cell order), so equal distances never depend on timing --,
 *                      the nnn (nnn - 1) / 2 values |R_a + R_b|^2 are formed, and the nnn / 2 smallest (ordered by value,
 *                      then pair index) are added in ascending order.  A centre with fewer than nnn partners gets 0, as
 *                      in LAMMPS.  No atomics on doubles: two reads of one state agree bit for bit.  MDP_EINVAL if a centre
 *                      has more than MDP_ADF_MAXNEIGH partners inside the cutoff (the short list a wave keeps in LDS): the
 *                      message names their number and asks for a smaller cutoff; no values are handed back and no centre is
 *                      ever truncated.  The context stays usable.  The other refusals as those of mdp_coord_read.
 *   mdp_centro_info:   out = {a measurement is on, its nnn, the centres with fewer than nnn partners at the last read, its
 *                      serial}.
 *   mdp_*_off:         releases the buffers. */
#define MDP_COORD_MAXCOL 32
#define MDP_CENTRO_MAXN 64
int mdp_coord_setup(mdp_ctx *ctx, double cutoff, int ncol, const int *jlo, const int *jhi, int groupbit);
int mdp_coord_read(mdp_ctx *ctx, int *tag /* [nlocal] */, double *values /* [nlocal][ncol] */);
int mdp_coord_info(mdp_ctx *ctx, long long out[4]);
int mdp_coord_off(mdp_ctx *ctx);
int mdp_centro_setup(mdp_ctx *ctx, int nnn, double cutoff, int groupbit);
int mdp_centro_read(mdp_ctx *ctx, int *tag /* [nlocal] */, double *values /* [nlocal] */);
int mdp_centro_info(mdp_ctx *ctx, long long out[4]);
int mdp_centro_off(mdp_ctx *ctx);

/* ---- per-atom structure: the common neighbour analysis (LAMMPS compute cna/atom Rc) ---------------------------------------
 * For a resident context with mdp_dd_setup (MDP_ESTATE otherwise), next to the measurements above and with their centres,
 * partners (here: neighbours) and binning.  For a centre with n neighbours inside the cutoff:
 *   n not 12 and not 14       pattern 5 (other), whatever n is: a centre with more than MDP_CNA_MAXNEAR neighbours is never
 *                             truncated into another pattern, and is counted (mdp_cna_info)
 *   every neighbour j         common = the neighbours k of the centre with |r_k - r_j|^2 < cutoff^2, the difference formed from
 *                             the two displacements from the centre; ncommon = |common|, nbonds = the pairs of common closer than
 *                             the cutoff, maxbond / minbond = the most / fewest such bonds one member of common takes part in
 *                             (0 / 8 for an empty set, as LAMMPS initialises them)
 *   n = 12                    12 x (4,2,1,1): 1 (fcc); 6 x (4,2,1,1) and 6 x (4,2,2,0): 2 (hcp); 12 x (5,5,2,2): 4 (icosahedral);
 *                             anything else 5
 *   n = 14                    6 x (4,4,2,2) and 8 x (6,6,2,2): 3 (bcc); anything else 5
 * Unlike LAMMPS the answer is formed from the current positions and not from a neighbour list of some age, it does not depend
 * on whether a neighbour is owned or a ghost, and cutoff + skin <= cutghost suffices (LAMMPS asks 2 Rc <= cutforce + skin).
 *   mdp_cna_setup:   MDP_EINVAL: cutoff <= 0 or not finite, cutoff + skin > the cutghost of mdp_dd_setup (see mdp_rdf_setup).
 *                    A second call replaces the first.
 *   mdp_cna_read:    blocking.  tag[i] and values[i] of this rank's nlocal owned atoms in the context's owned order: the pattern
 *                    1 .. 5 as a double, 0 for an atom outside the group.  Integers throughout: two reads of one state agree
 *                    bit for bit.  The refusals as those of mdp_coord_read.
 *   mdp_cna_counts:  out[p] = this rank's group atoms with pattern p = 0 .. 5 at the last read (out[0] is always 0), counted on
 *                    the device in 64-bit integers; all 0 before the first read.  MDP_ESTATE without a setup.
 *   mdp_cna_info:    out = {a measurement is on, 0, the centres with more than MDP_CNA_MAXNEAR neighbours at the last read, its
 *                    serial}.
 *   mdp_cna_off:     releases the buffers. */
#define MDP_CNA_MAXNEAR 16
int mdp_cna_setup(mdp_ctx *ctx, double cutoff, int groupbit);
int mdp_cna_read(mdp_ctx *ctx, int *tag /* [nlocal] */, double *values /* [nlocal] */);
int mdp_cna_counts(mdp_ctx *ctx, long long out[6]);
int mdp_cna_info(mdp_ctx *ctx, long long out[4]);
int mdp_cna_off(mdp_ctx *ctx);

/* ---- binned mass, momentum and kinetic energy: temperature, density and flow profiles (LAMMPS compute chunk/atom bin/1d|2d|3d
 * with compute temp/chunk, vcm/chunk, fix ave/chunk), in integers ----------------------------------------------------------
 * For a resident context with mdp_dd_setup (MDP_ESTATE otherwise).  Nothing a step, a list build, msd or rdf reads is touched.
 *   mdp_profile_setup:    bins over the box of mdp_dd_setup in ndim = 1 .. 3 distinct dimensions dim[k] in {0, 1, 2} with
 *                         nbin[k] >= 1 bins each, nbin[0] * .. <= MDP_PROFILE_MAXBINS rows (MDP_EINVAL otherwise).  An owned
 *                         atom with fractional coordinate s_d (Domain::x2lamda, triclinic included) has b_d = (int)
 *                         floor(s_d nbin_d), wrapped ((b % n) + n) % n in a periodic dimension (an atom that drifted out of
 *                         the box since the last remap lands where its image would) and clamped to 0 .. n - 1 in a
 *                         non-periodic one; row = the first named dimension slowest.  groupbit: 0 every owned atom, else the
 *                         atoms whose mask (mdp_md_set_mask) has the bit.  A second call replaces the first.
 *   The terms of an atom with mass m and full-step velocity v: t = (m, m vx, m vy, m vz, m (v . v)); both reads first
 *   complete a final half-kick the host deferred.
 *   mdp_profile_range:    blocking.  out[k] = this rank's max |t_k| over the group's owned atoms (0 without one).
 *   mdp_profile_exponent: pure host function.  0 for range == 0, else 61 - ceil(log2(max(natoms_total, 2))) - E with range < 2^E
 *                         (E the frexp exponent): natoms_total * (range * 2^e + 1/2) < 2^62, so no sum of natoms_total
 *                         quantised terms overflows.  Every rank must use the exponents of the GLOBAL range maximum.
 *   mdp_profile_sums:     blocking.  count[b] = the group's owned atoms of this rank in row b; sums[b][k] = the sum of
 *                         llrint(ldexp(t_k, exponent[k])) over them as 64-bit integers.  All integers, no float atomics:
 *                         two reads of one state agree exactly, and the sum over the bricks equals the one-brick table bit
 *                         for bit.  MDP_EINVAL when an |ldexp(t_k, exponent[k])| >= 2^62 / max(nlocal, 1) (the message names the
 *                         column); MDP_ESTATE without a setup, or with a group and no mask that covers the current atoms.
 *   mdp_profile_info:     out = {a measurement is on, its rows, its ndim, its serial}; the serial as that of mdp_rdf_info.
 *   mdp_profile_off:      releases the buffers. */
#define MDP_PROFILE_W 5
#define MDP_PROFILE_MAXBINS (1 << 20)
int mdp_profile_setup(mdp_ctx *ctx, int ndim, const int *dim, const int *nbin, int groupbit);
int mdp_profile_range(mdp_ctx *ctx, double out[MDP_PROFILE_W]);
int mdp_profile_exponent(double range, long long natoms_total);
int mdp_profile_sums(mdp_ctx *ctx, const int exponent[MDP_PROFILE_W], long long *count, long long *sums);
int mdp_profile_info(mdp_ctx *ctx, long long out[4]);
int mdp_profile_off(mdp_ctx *ctx);

/* ---- the heat current J = sum (ke_i + pe_i) v_i + sum W_i . v_i (LAMMPS compute heat/flux fed ke/atom, pe/atom and
 * stress/atom NULL virial), from the per-atom tallies a compute left on the device -------------------------------------------
 * For a resident context (MDP_ESTATE otherwise).  pe_i and W_i (xx yy zz xy xz yz) are what mdp_md_compute(eflag | 2,
 * vflag | 4) -- or mdp_dd_comm_step_begin / _end with those flags -- tallied, in the reference's split (v_tally2/3,
 * ev_tally3: not the centroid form).  In resident mode the shares of periodic self-images end on their owners inside the
 * tallying compute.  The context remembers the flags of its last finished compute; a new compute, anything that moves the
 * atoms (an integrate call, mdp_md_upload_x), a reneighbouring that re-orders them and mdp_md_setup make the tallies stale until the next
 * tallying compute.  A final half-kick -- also the one a read here completes -- leaves them valid.
 *   mdp_heatflux_sums:     blocking.  This rank's sums over the owned atoms (groupbit != 0: those with mask & groupbit) with
 *                          full-step velocities (a final half the host deferred is completed first):
 *                          out[0..2] = sum (1/2 mvv2e m v.v + eatom_i) v_i, out[3..5] = sum W_i . v_i
 *                          (x: W0 vx + W3 vy + W4 vz, y: W3 vx + W1 vy + W5 vz, z: W4 vx + W5 vy + W2 vz),
 *                          out[6] = the atoms summed, out[7] = sum (ke_i + eatom_i).  Extensive, not divided by the volume;
 *                          the caller adds over ranks and forms LAMMPS' vector [out[0..2] + out[3..5], out[0..2]].  Fixed
 *                          order, no float atomics: two reads of one state agree bit for bit.
 *   mdp_md_download_vatom: blocking.  vatom [nlocal][6] of the owned atoms in device order, the sibling of the eatom
 *                          argument of mdp_md_download.
 * Both: MDP_ESTATE unless the last finished compute ran with MDP_EFLAG_ATOM and MDP_VFLAG_ATOM and its tallies are not
 * stale; MDP_ENOTIMPL for an aeam brick of several ranks whose angular centres may reach a remote ghost (mdp_md_aeam_state
 * out[3] == 1): the thirds three-body terms put on remote ghosts would need a reverse exchange of 7 doubles per ghost.
 * mdp_heatflux_sums: MDP_ESTATE with a group bit and no mask that covers the current atoms. */
int mdp_heatflux_sums(mdp_ctx *ctx, int groupbit, double out[8]);
int mdp_md_download_vatom(mdp_ctx *ctx, double *vatom /* [nlocal][6], device order */);

/* per-phase device time of the last compute in ms (HIP events on the compute stream):
 * rebomos: [0]=REBO centre kernels of the lane-group classes, [1]=the general kernel (centres that outgrew their lane
 * group since the list build), [2]=row pruning (0 unless one was due), [3]=LJ+gather kernel;
 * aeam: [0]=density of the metal centres (tile kernel), [1]=density of the angular centres, [2]=embedding,
 * [3]=force tile kernel (incl. force_clear), [4]=angular three-body forces.
 * Enabled by mdp_set_timing(ctx,1). */
int mdp_set_timing(mdp_ctx *ctx, int on);
int mdp_get_timing(mdp_ctx *ctx, double ms[8]);

#ifdef __cplusplus
}
#endif
#endif /* MDPAIR_HIP_H */
