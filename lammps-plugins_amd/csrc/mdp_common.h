// mdp_common.h -- internal context and helpers of libmdpair_hip.so (gfx950 only)
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "devbuf.h"
#include "mdpair_hip.h"

#define MDP_NEIGHMASK 0x1FFFFFFF
// global energy/virial accumulators: acc[0..15] final values (0 eng, 1..6 virial, 7 KE, 8 maxdisp2),
// followed by MDP_ACC_SLOTS partial slots of MDP_ACC_STRIDE doubles each
#define MDP_CLUSTER 2
static_assert(MDP_CLUSTER == 1 || MDP_CLUSTER == 2, "the Lennard-Jones kernels are instantiated for 1- and 2-atom clusters only");
#define MDP_TILE 16 // clusters per tile of the tile rows (tiles.hip) = 256 threads / 16 lanes per cluster
#define MDP_ACC_SLOTS 512
#define MDP_ACC_STRIDE 16
// REBO centre classes: lane-group size (4, 8, 12, 16, 32) x element, x {interior, boundary}: classes 10..19 hold the
// centres whose candidate set reaches a REMOTE ghost (multi-GPU runs); the interior ones run while the halo is in flight
#define MDP_NOVF_LISTS 7 // {count, ids ...} lists in mdp_ctx::ovf, counts zeroed with the accumulators of every compute: [0] centres for the
                         // general kernel, [1..4] the lane-per-centre kernel's overflow per (part, element), [5] tiles with a pair on
                         // the cubic Lennard-Jones spline, [6] those of them whose pair queues overflowed (rows walked after all)
#define MDP_NCLASS 20
#define MDP_NCLASS_HALF 10

// every device allocation of the library: MdpBuf (devbuf.h) on the HIP allocator.  copy: the old contents into a grown
// buffer, complete on return
struct MdpHipMem {
  using error = hipError_t;
  using stream = hipStream_t;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void **q, size_t bytes) { return hipMalloc(q, bytes); }
  static void free(void *p) { (void) hipFree(p); }
  static hipError_t copy(void *dst, const void *src, size_t bytes, hipStream_t s)
  {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
  }
};
template <typename T> using DevBuf = MdpBuf<T, MdpHipMem>;

// REBO-MoS parameters as the kernels see them: pair tables flattened [ti*2+tj]
struct RebomosDev {
  double rcmin[4], rcmax[4], rcmaxsq[4], rcinv[4]; // rcinv = 1/(rcmax-rcmin)
  double Q[4], alpha[4], A[4], B[4], beta[4];
  double b[2][7], bg[2][7], a[2][4];
  // LJ: thresholds in rsq space chosen so that the branch taken is bit-identical to the
  // reference's comparisons on rij = sqrt(rsq) (pair_rebomos.cpp:518-532)
  double lj_rsq_lo[4];  // smallest rsq with sqrt(rsq) >= rcLJmin
  double lj_rsq_hi[4];  // largest  rsq with sqrt(rsq) <= rcLJmax
  double lj_rsq_sw[4];  // smallest rsq with sqrt(rsq) >= 0.95*sigma
  double lj1[4], lj2[4], lj3[4], lj4[4];
  double ljc2[4], ljc3[4], rcLJmin[4]; // cubic inner spline (pair_rebomos.cpp:533-543)
  double cand_cutsq[4];                // (rcmax+skin)^2 : REBO candidate list
  double ljlist_cutsq[4];              // (rcLJmax+skin)^2 : trimmed LJ list
};

// The style-level displacement checks of a resident run (has an atom moved half the inner skin since the style's lists
// were built / half the pruning buffer since the rows were pruned?) ride in kernels that touch the positions anyway:
// owned atoms in the integrate kernel, remote ghosts in the halo unpack; periodic self-images move with their owners.
// Flag words are pinned host memory, two sets used alternately (the words of step n are read during step n+1, after
// the integrate kernel of step n+1 was queued -- never in the step that writes them, which would be a host wait on a
// kernel just launched): [0] beyond the list trigger [1] beyond half the inner skin [2] beyond
// the pruning trigger [3] beyond half the buffer; [4..7] the same for remote ghosts.
// Reference positions of the displacement checks (at the last reneighboring, style-list build, row pruning): single
// precision -- the triggers have margins of 0.07-0.1 A, a float resolves 6e-5 A at |x| = 1000 A -- which takes 36 of
// the 216 bytes per atom out of the integrate kernel.
typedef float mdp_hold_t;
struct MdpStyleCheck {
  const mdp_hold_t *xa = nullptr, *xp = nullptr; // positions at the style-list build / at the last row pruning, [nall][3]
  double trig_a = 0, hard_a = 0, trig_p = 0, hard_p = 0; // squared distances
  int *flag = nullptr;
  // accumulators reset by the same kernel (mdp_acc_begin of the compute that follows): acc[0..nacc), flags, ovf[0]
  double *acc = nullptr;
  int nacc = 0;
  int *flags = nullptr, *ovf = nullptr;
  int ovf_stride = 0; // the MDP_NOVF_LISTS list counters (five overflow lists, two lists of cubic-spline tiles) sit at ovf[k * ovf_stride]
};
struct MdpStyleCheckMeta {
  bool has_style = false, has_prune = false;
  long long build_epoch = -1;
  int prune_epoch = -1;
};
// The deferred triggers are read one compute late, so they fire early by these margins (Angstrom; two steps of motion
// for the pruned rows: in a multi-GPU run the owned atoms are checked before the halo of the same step arrives)
constexpr double kStaleMargin = 0.1;
constexpr double kPruneMargin = 0.07;

// uniform Cartesian bin grid over the bounding box of owned+ghost atoms
struct MdpGrid {
  double lo[3], inv[3];
  int n[3];
  int range; // stencil half width in cells: range * cell width >= the cutoff the grid was made for
};

// The cell of a position on the grid of mdp_measure_bin.  It clamps: an atom that has drifted up to skin / 2 past the bounding
// box of the last reneighbouring lands in an edge cell.  Cells are >= cutoff / 2 wide and the box is padded by more than
// skin, so the atom is less than one cell outside and the 5-cell stencil around the edge cell still reaches every partner
// within the cutoff.
__device__ __forceinline__ int mdp_bin_cell_index(const MdpGrid &g, const double4 &x, int &cx, int &cy, int &cz)
{
  cx = (int) ((x.x - g.lo[0]) * g.inv[0]);
  cy = (int) ((x.y - g.lo[1]) * g.inv[1]);
  cz = (int) ((x.z - g.lo[2]) * g.inv[2]);
  cx = cx < 0 ? 0 : (cx >= g.n[0] ? g.n[0] - 1 : cx);
  cy = cy < 0 ? 0 : (cy >= g.n[1] ? g.n[1] - 1 : cy);
  cz = cz < 0 ? 0 : (cz >= g.n[2] ? g.n[2] - 1 : cz);
  return cx + g.n[0] * (cy + g.n[1] * cz);
}

// The reference sizes everything from the potential file (pair_aeam.cpp:752-872; the bundled AlSi.aeam has two
// elements), and so does this library.  Up to MDP_AEAM_MAXT atom types the parameters of the type pairs also ride in
// the kernel arguments (1.8 KB of the 4 KB a launch may carry), where the tile kernels and the templated CSR kernels read
// them as scalars at fixed offsets; with more types only the block in device memory (g_*) exists and the generic CSR
// kernels (PairPar<0>) serve every step.
#define MDP_AEAM_MAXT 8
#define MDP_AEAM_MAXTYPES 64 // (a sanity bound on what a file may declare, not a table size)
struct AeamDev {
  int ntypes, nelements, nnonangular, nrhomax, nrmax;
  // per type pair [(ti-1)*ntypes + (tj-1)], filled when ntypes <= MDP_AEAM_MAXT
  double cut[MDP_AEAM_MAXT * MDP_AEAM_MAXT], rdr[MDP_AEAM_MAXT * MDP_AEAM_MAXT];
  int nr[MDP_AEAM_MAXT * MDP_AEAM_MAXT], t2rhor[MDP_AEAM_MAXT * MDP_AEAM_MAXT], t2z2r[MDP_AEAM_MAXT * MDP_AEAM_MAXT];
  double rdrho[MDP_AEAM_MAXT];
  int nrho[MDP_AEAM_MAXT], t2frho[MDP_AEAM_MAXT];
  // the same in device memory for any number of types: [ntypes*ntypes] / [ntypes]
  const double *g_cut, *g_rdr, *g_rdrho;
  const int *g_nr, *g_t2rhor, *g_t2z2r, *g_nrho, *g_t2frho;
  const double *frho, *rhor, *z2r; // device spline tables [table][row][7]
  const double4 *rhor_v4, *rhor_d4, *z2r_v4, *z2r_d4; // the same rows as aligned {c3..c6} / {c0..c2,0} records
  const double2 *rhor_ys, *z2r_ys; // [table][nrmax+1] (value, slope) = columns 6 and 5 of a row: the persistent tile kernels' tables
  const double2 *pair_d6; // [ntypes*ntypes][nrmax+1][3]: {rho' c0 c1 | rho' c2, phi' c0 | phi' c1 c2} of the pair type, 48 B per row
};

// blocks of `per` threads (or work items) that cover n
inline int nblk(long long n, int per = 256) { return (int) ((n + per - 1) / per); }

// butterfly sum over W consecutive lanes (W a power of two <= 64): every lane of the group ends with the total
template <int W> __device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Work items that are neighbours
// in space (consecutive along the Hilbert curve) share most of what they gather, so every XCD is given one
// contiguous stretch of the items instead of every eighth one.
__device__ __forceinline__ int xcd_contiguous(const int b, const int n)
{
  const int q = n >> 3, r = n & 7, xcd = b & 7, idx = b >> 3;
  return xcd * q + (xcd < r ? xcd : r) + idx;
}

// 30-bit key of a cell (10 bits per axis) along a 3-D Hilbert curve (Skilling, "Programming the Hilbert curve":
// axes -> transposed index).  A Hilbert curve has no jumps: any run of consecutive keys is a compact blob, which
// is what bounds the neighbour unions of the tile lists.
__device__ __forceinline__ unsigned mdp_hilbert30(unsigned x0, unsigned x1, unsigned x2)
{
  constexpr int B = 10;
  unsigned X[3] = {x0, x1, x2};
  for (unsigned Q = 1u << (B - 1); Q > 1; Q >>= 1) {
    const unsigned P = Q - 1;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      if (X[d] & Q)
        X[0] ^= P;
      else {
        const unsigned t = (X[0] ^ X[d]) & P;
        X[0] ^= t;
        X[d] ^= t;
      }
    }
  }
  X[1] ^= X[0];
  X[2] ^= X[1];
  unsigned t = 0;
  for (unsigned Q = 1u << (B - 1); Q > 1; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1;
  X[0] ^= t;
  X[1] ^= t;
  X[2] ^= t;
  unsigned key = 0;
  for (int b = B - 1; b >= 0; b--)
#pragma unroll
    for (int d = 0; d < 3; d++) key = (key << 1) | ((X[d] >> b) & 1u);
  return key;
}

// ---- brick domain decomposition (domain.hip): geometry as the kernels see it
struct DdGeom {
  double lo[3];
  double h[6], hinv[6]; // LAMMPS Domain::h order: xprd, yprd, zprd, yz, xz, xy
  int g[3];             // bricks per dimension
  int me[3], rank, nranks;
  double cutl[3];       // ghost-shell width in lamda (fractional) units
  int ns[3];            // periodic image shifts tested per dimension: -ns .. ns
  int self_remote;      // testing: periodic self-images travel through the transport (to the rank itself)
  int nonper[3];        // 1: no periodic images / no wrap in this dimension (slab, free surface)
};

// fractional (lamda) coordinates of a position in the box of mdp_dd_setup (Domain::x2lamda), triclinic included
__device__ __forceinline__ void dd_x2lamda(const DdGeom &G, const double x, const double y, const double z, double lam[3])
{
  const double d0 = x - G.lo[0], d1 = y - G.lo[1], d2 = z - G.lo[2];
  lam[0] = G.hinv[0] * d0 + G.hinv[5] * d1 + G.hinv[4] * d2;
  lam[1] = G.hinv[1] * d1 + G.hinv[3] * d2;
  lam[2] = G.hinv[2] * d2;
}

// LAMMPS' 32-bit imageint:(ix + 512) | (iy + 512) << 10 | (iz + 512) << 20; a field wraps modulo 1024
constexpr int kImgBits = 10, kImgMask = 1023, kImgBias = 512;
// unwrapped position x + h . image of an atom, the roundings written out (both kernels that form it give the same bits)
__device__ __forceinline__ void mdp_unwrap(const DdGeom &G, const double4 &x, const int image, double xu[3])
{
  const double ix = (double) ((image & kImgMask) - kImgBias), iy = (double) (((image >> kImgBits) & kImgMask) - kImgBias),
               iz = (double) (((image >> 2 * kImgBits) & kImgMask) - kImgBias);
  xu[0] = fma(G.h[4], iz, fma(G.h[5], iy, fma(G.h[0], ix, x.x)));
  xu[1] = fma(G.h[3], iz, fma(G.h[1], iy, x.y));
  xu[2] = fma(G.h[2], iz, x.z);
}

struct MdpDomain {
  bool on = false;
  DdGeom G;
  double cutghost = 0.0;
  std::vector<int> mig_send, bord_send, bord_recv; // per rank
  int mig_total = 0, nself = 0, nsend = 0, nrecv = 0, nent = 0;
  int nlocal_old = 0, nghost_old = 0;
  long long reneighbors = 0;
  DevBuf<int> dest, counters, idx_a, idx_b, ent_atom, ent_code, ent_cnt, ent_off, sendlist, type_tmp, tag_tmp, mask_tmp, image_tmp;
  DevBuf<unsigned long long> key_a, key_b;
  DevBuf<double> sendshift, v_tmp;
  DevBuf<double4> xq_tmp;
  // deferred displacement trigger of the host-level skin (neigh_modify check yes)
  hipEvent_t ev_moved = nullptr, ev_moved_ref = nullptr; // (_ref: ev_moved, or the style-check event behind the same kernel)
  bool moved_pending = false;
  // RCCL transport inside the library (comm_rccl.hip)
  void *nccl_comm = nullptr;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_packed = nullptr, ev_arrived = nullptr, ev_lead = nullptr;
  DevBuf<double> sbuf, rbuf, abuf; // abuf: the all-reduce's own words
  bool fwd_pending = false;        // a position exchange is in flight between _forward_begin and _forward_end
  int aeam_pending = 0;            // the aeam fp (1) / fp + ghost force (2) exchange is in flight
  DevBuf<int> cnt_dev;
  // The collective `check yes` decision rides with the halo (mdp_dd_comm_step_begin / _end): the integrate kernel of a
  // step leaves "an owned atom of this rank has moved beyond the trigger" in a device word (two words alternate: the
  // kernel sets one and clears the other), an all-gather of that word follows the position exchange on the
  // communication stream, the halo unpack reduces the ranks' words into a pinned word, and every rank reads the SAME
  // answer at its next step -- no blocking thermo call, no host-side collective.
  DevBuf<double> flagbuf;          // [0..1] this rank's word of the even / odd steps, [2 .. 2 + nranks) the ranks' words as gathered
  int flag_par = 0;
  hipEvent_t ev_glob = nullptr, ev_glob_ref = nullptr; // (_ref: ev_glob, or the style-check event recorded behind the same kernel)
  bool glob_pending = false;
  bool step_mode = false;          // the host drives whole steps (mdp_dd_comm_step_begin / _end): the words are gathered every step
  bool fwd_gathered = false;       // the all-gather of the words was queued behind the position exchange in flight
  bool fresh_ghosts = false;       // the border exchange of a reneighboring carried the current positions
  bool ghost_forces = true;        // aeam: some rank has an angular centre next to a remote ghost (decided per reneighboring)
  long long dangerous = 0;         // step mode: checks that saw an owned atom beyond half the skin
  long long steps_phased = 0;      // aeam steps whose exchanges travelled behind the interior tiles
  // How a step orders its compute against its exchanges (mdp_dd_comm_step_begin / _end), chosen from measurements on
  // the machine the run is on (comm_rccl.hip, "overlap policy"):
  //   0 split     the work that needs no remote ghost of this step is launched behind the start of the exchange
  //   1 lead      as 0, and the compute stream waits until the RCCL kernel of the exchange has started (comm_lead)
  //   2 blocking  exchange first, then the whole compute in its one-GPU order
  //   3 first     rebomos only: of the interior work only the first kernel (lane-per-centre) runs behind the exchange
  //   4 inline    as blocking, with the position exchange queued on the context's own stream (no second stream, no events)
  int ov_policy = -1;              // the choice; -1 while the trial runs
  int ov_forced = -2;              // MDP_OVERLAP_POLICY: -2 not read yet, -1 auto, >= 0 fixed
  int ov_cur = 0;                  // policy of the step in flight
  bool lead = false;               // (policy 1 of the step in flight)
  long long ov_step = 0;           // steps the trial has seen
  double ov_sum[5] = {0, 0, 0, 0, 0}; // device time of the measured steps per policy, ms
  int ov_cnt[5] = {0, 0, 0, 0, 0};
  double ov_mean[5] = {0, 0, 0, 0, 0};
  bool inline_x = false, fwd_inline = false; // (policy 4 of the step in flight; how the exchange in flight was queued)
  hipEvent_t ov_ev[4][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  int ov_slot_pol[4] = {-1, -1, -1, -1}; // policy of the step a slot's event pair brackets (-1: free)
  int ov_slot = -1;                // slot of the step in flight (-1: not measured)
};

constexpr int MDP_UP_RING = 2;      // host-mode upload: pinned staging chunks in flight
constexpr int MDP_DOWN_CHUNKS = 8;  // host-mode download: pieces of the force array
// Nose-Hoover chain thermostat (nhc.hip): the chain lives in st on the device; the host keeps the step counter and the
// ramp of the current run
struct MdpNhc {
  bool on = false;
  bool need_setup = false;  // the next initial half sets the masses up again from the velocities (FixNH::setup)
  mdp_nhc_config cfg;
  long long first = 0, last = 0, step = 0;
  double tt = 0.0;          // target temperature of the current step
  DevBuf<double> st;        // [MDP_NHC_STATE_LEN] state (mdp_nhc_state layout), then Q[8], then the scale factor S
  DevBuf<double> part;      // per-block partial sums of m v^2 (fixed slots: the reduction is bitwise reproducible)
};
static constexpr int kNhcQ = MDP_NHC_STATE_LEN, kNhcS = MDP_NHC_STATE_LEN + MDP_NHC_MAXCHAIN, kNhcWords = kNhcS + 1;
// Langevin thermostat (langevin.hip): the host keeps the step counter and the ramp; the per-type factors, the mean of
// the random parts (zero yes) and the tally live on the device
struct MdpLangevin {
  bool on = false;
  bool need_setup = false;  // the next initial half applies the setup force of the run first (Fix::setup)
  long long first = 0, last = 0, step = 0; // step: the step of the forces the next post_force is applied to
  double tab_dt = 0.0, tab_ftm2v = 0.0;    // what the factors in st were computed for
  // nbath baths (>= 1 while on) share first / last / step / need_setup.  One bath (mdp_langevin_setup) acts on the group
  // of mdp_langevin_group and its kernels are the NB = 1 instantiations; several (mdp_langevin_baths) act on disjoint
  // groups, bath k on bit[k], in the NB = MDP_LANGEVIN_MAXBATH instantiations.  NB is the slot count of everything below.
  int nbath = 0;
  mdp_langevin_config cfg[MDP_LANGEVIN_MAXBATH];
  int bit[MDP_LANGEVIN_MAXBATH] = {0, 0, 0, 0};
  bool any_zero = false, any_tally = false;
  DevBuf<double> st;        // bath k at st + k * kLgvWords: [0..16) gfactor1, [16..32) gfactor2, [32..35) mean, [35] energy, [36] E of the last step
  DevBuf<double> part;      // per-block partial sums (zero: 3 NB per block, [bath][3]; then tally: NB per block)
  bool disjoint_checked = false; // the current mask has been counted for atoms in more than one bath
  DevBuf<int> overlap;           // [1] that count
  bool many() const { return on && nbath > 1; }
  bool sums() const { return on && (any_zero || any_tally); } // one rank only
};
static constexpr int kLgvG2 = 16, kLgvMean = 32, kLgvE = 35, kLgvElast = 36, kLgvWords = 37;
// Constant-flux heat sources (heat.hip): the host keeps the step counter and which sources are due; the sums, the scale
// factors and the latched error live on the device.  st: source k keeps kHeatWords words at st + k * kHeatWords -- its
// MDP_HEAT_STATE_LEN state words (mdp_heat_state layout), then the scale and (scale - 1) vcm of the pass in flight (1 and 0
// for a source that is not due); behind the sources the error latch (kHeatErr: 1 once latched, then its source)
struct MdpHeat {
  bool on = false;
  bool started = false;     // an initial half has run since mdp_heat_run: the next final half completes a step of this run
  bool counted = false;     // the current mask has been counted (atoms in two sources, outside the integrate group, per source)
  bool mass_due = false;    // the next pass sums M again (set-up, mask upload)
  int nsrc = 0;
  mdp_heat_config cfg[MDP_HEAT_MAXSRC];
  int bit[MDP_HEAT_MAXSRC] = {0, 0, 0, 0};
  long long step = 0;       // the step the last initial half began
  DevBuf<double> st;        // [MDP_HEAT_MAXSRC * kHeatWords + 2]
  DevBuf<double> part;      // per-block partial sums, kHeatW per block (fixed slots)
  DevBuf<int> count;        // [2 + MDP_HEAT_MAXSRC] the counts of a set-up or mask upload
};
static constexpr int kHeatScale = 0, kHeatVcm = 1, kHeatKe = 4, kHeatM = 5, kHeatN = 6, kHeatErrStep = 7, kHeatS = 8, kHeatVsub = 9,
                     kHeatWords = 12, kHeatErr = MDP_HEAT_MAXSRC * kHeatWords, kHeatTotal = kHeatErr + 2;
static constexpr int kHeatW = 5 * MDP_HEAT_MAXSRC; // per source: sum m v.v, m vx, m vy, m vz, m
// Post-force stages: the device fixes that add a force in front of every kick that first consumes a compute's forces
// (the indenters, then the tether springs, then the prescribed group forces: kMdpStages below, postforce.hip).  The host keeps the configuration, the number
// of initial halves since the stage's _run and whether the current forces have had the stage's pass; the sums live on the
// device.  What every stage keeps:
static constexpr int kStageSlots = 4; // indenters, springs, group-force slots of one context
static_assert(MDP_INDENT_MAX == kStageSlots && MDP_SPRING_MAX == kStageSlots && MDP_GFORCE_MAX == kStageSlots, "a stage has four slots");
struct MdpPostForce {
  bool on = false;
  bool applied = false;     // the forces the context holds have had this stage's pass.  Set by mdp_postforce_apply, cleared
                            // behind every initial half (mdp_postforce_count_step) and by the stage's _setup / _run
                            // (mdp_postforce_restart), nowhere else
  int n = 0;                // slots that are on
  int bit[kStageSlots] = {0, 0, 0, 0}; // their group bits (0: every owned atom)
  long long first = 0;      // the step of the stage's _run
  long long nhalf = 0;      // initial halves since: the current forces are those of step first + nhalf
  DevBuf<double> st;        // the state words of every slot (the stage's _state layout)
  DevBuf<double> part;      // per-block partial sums (fixed slots [block][slot][5])
};
// Indenters (indent.hip): LAMMPS fix indent with a constant velocity, added into f by the stage's pass.  st: indenter k
// keeps its MDP_INDENT_STATE_LEN state words (mdp_indent_state layout) at st + k * MDP_INDENT_STATE_LEN; part: kIndW per block
struct MdpIndent : MdpPostForce {
  mdp_indent_config cfg[MDP_INDENT_MAX];
};
static constexpr int kIndW = 5 * MDP_INDENT_MAX; // per indenter: energy, the atoms' fx, fy, fz, atoms in contact
// Tether springs (spring.hip): LAMMPS fix spring tether with a tether point at constant velocity, taken off f by the
// stage's pass, behind the indenters'.  st ([kSprTotal]): spring k keeps its MDP_SPRING_STATE_LEN state words
// (mdp_spring_state layout) at st + k * MDP_SPRING_STATE_LEN; behind the springs, F / M of the pass in flight (kSprF + 4 k:
// x, y, z and a spare word); part: kSprW per block
struct MdpSpring : MdpPostForce {
  mdp_spring_config cfg[MDP_SPRING_MAX];
  DevBuf<int> cpart;        // per-block atom counts, MDP_SPRING_MAX per block
  DevBuf<int> count;        // [2 MDP_SPRING_MAX] the counts of a set-up: atoms per spring, those with a mass
};
static constexpr int kSprW = 5 * MDP_SPRING_MAX; // per spring: sum m xu, m yu, m zu, m_hi, m_lo (m = m_hi + m_lo, spring.hip)
static constexpr int kSprF = MDP_SPRING_MAX * MDP_SPRING_STATE_LEN, kSprTotal = kSprF + 4 * MDP_SPRING_MAX;
// Prescribed group forces (gforce.hip): LAMMPS fix setforce, addforce and aveforce with constant values, written into f by
// the stage's pass, behind the springs'.  st: slot k keeps its MDP_GFORCE_STATE_LEN state words (mdp_gforce_state layout) at
// st + k * MDP_GFORCE_STATE_LEN -- words [6..9) of an AVE slot are what the apply kernel writes; part: kGfW per block
struct MdpGforce : MdpPostForce {
  mdp_gforce_config cfg[MDP_GFORCE_MAX];
  bool counted = false;     // the AVE sharing rule has been counted for the current mask (gforce.hip)
  DevBuf<int> cpart;        // per-block atom counts, MDP_GFORCE_MAX per block
  DevBuf<int> count;        // [MDP_GFORCE_MAX + MDP_GFORCE_MAX^2] the counts of a set-up or mask upload
};
static constexpr int kGfW = 5 * MDP_GFORCE_MAX; // per slot: the sums of fx, fy, fz before the slot acted, its energy, a spare word
// FIRE minimiser (fire.hip): the control block lives in st on the device; the host keeps the configuration and what it
// has queued.  Control block, in doubles (flags and counters as whole numbers):
enum MdpFireWord {
  kFireDtv = 0,   // the step of this iteration (dt, shortened by dmax)
  kFireDtvPrev,   // ... of the iteration before (halfstepback)
  kFireS1,        // mixing: v = s1 v + s2 f
  kFireS2,
  kFireMix,       // 1: P > 0 in this iteration
  kFireZero,      // 1: P <= 0 in this iteration (half step back, v = 0)
  kFireDt,
  kFireAlpha,
  kFireIter,      // iterations done (the one in flight included once its control kernel has run)
  kFireLastNeg,   // iteration of the last P <= 0
  kFireNneg,      // number of P <= 0 so far
  kFireFF,        // sum f.f as the last control kernel saw it (the forces of the iteration before)
  kFireStop,      // latched MDP_FIRE_* stop code, 0 while running
  kFireNeval,     // force evaluations of the iterations
  kFireEprev,     // energies of the last two evaluations (etol > 0)
  kFireElast,
  kFireVdotF,     // P of this iteration
  kFireFFnow,     // sum f.f of the current forces (a state read refreshes it)
  kFireWords
};
struct MdpFire {
  bool on = false;
  mdp_fire_config cfg;
  double dt0 = 0.0;            // the time step the minimisation started from (dtmax = tmax dt0, dtmin = tmin dt0)
  double e_initial = 0.0, fnorm_initial = 0.0;
  double e_cache = 0.0;        // etol == 0: the energy of the last state read ...
  long long e_cache_iter = -1; // ... and the iteration it belongs to
  long long reneighbors0 = 0;  // MdpDomain::reneighbors at setup
  long long late = 0;          // displacement checks that saw an atom beyond half the skin already
  DevBuf<double> st;           // [kFireWords]
  DevBuf<double> part;         // per-block partials: 3 sums per block, then one maximum per block
  DevBuf<double> fsave;        // a state read's energy compute leaves the forces as it found them
};

// A measurement a context holds one of per kind (msd, rdf, profile): whether it is set up, and which setup of this process
// it is (mdp_measure_start; mdp_*_info hands the serial out, so that a caller knows its own setup from another's)
struct MdpMeasure {
  bool on = false;
  long long serial = 0;
};
// mean-squared displacement (msd.hip): the origins of the WHOLE system by tag on every rank, so nothing has to migrate
struct MdpMsd : MdpMeasure {
  int ntag = 0, gbit = 0;
  DevBuf<double> x0;   // [ntag][3] unwrapped origin of the atom with tag t at [t - 1]
  DevBuf<double> xu;   // [nlocal][3] unwrapped positions (mdp_md_download_unwrapped)
  DevBuf<double> part; // per-block partials, kMsdW per block, then the kMsdW sums
};
// The binning of a pair or angle measurement (measure_bin.hip): ALL atoms of the brick, owned and ghost, on a grid of its own.
// Nothing here is shared with the list builders, so a read leaves the run's scratch alone.
struct MdpBinning {
  DevBuf<unsigned> key_a, key_b;   // cell of every atom, before and after the sort
  DevBuf<int> val_a, perm, code;   // atom indices before / after the sort; type, membership and ownership per atom
  DevBuf<int> cell_start;          // [ncell + 1]
  DevBuf<double4> rec;             // [nall] {x, y, z, code} in cell order
  DevBuf<char> sort_tmp;
  void release()
  {
    key_a.release();
    key_b.release();
    val_a.release();
    perm.release();
    code.release();
    cell_start.release();
    rec.release();
    sort_tmp.release();
  }
};
constexpr int kBinTypes = 16; // type codes 0 .. 15 of a record: 0 = not a member, t = LAMMPS type t
constexpr int kBinOwned = 32; // code bit: an owned atom (a lane that counts)
// pair-distance histograms (rdf.hip): the binning and the counters of a read
struct MdpRdf : MdpMeasure {
  int nbin = 0, npair = 0, ntypes = 0, ntag = 0; // ntag 0: every atom is a member
  double cutoff = 0.0;
  DevBuf<unsigned char> member;    // [ntag] membership of the atom with tag t at [t - 1], the WHOLE system on every rank
  DevBuf<int> tab;                 // column masks per (type i, type j), then the i and j masks per type
  MdpBinning bin;
  DevBuf<unsigned long long> out;  // [npair][nbin] histogram, then icount / jcount / dup [MDP_RDF_MAXPAIR] each, then the bad tags
};
// bond-angle histograms (adf.hip): the same, with the shells of every triple
struct MdpAdf : MdpMeasure {
  int nbin = 0, ntriple = 0, ntypes = 0, ntag = 0, ordinate = 0;
  double rmax = 0.0;               // the largest outer radius: what the grid and the ghost shell have to cover
  DevBuf<unsigned char> member;    // as MdpRdf::member
  DevBuf<double> tab;              // squared shell radii [4][MDP_ADF_MAXTRIPLE], then the triple masks per type (adf.hip)
  MdpBinning bin;
  DevBuf<unsigned long long> out;  // [ntriple][nbin] histogram, icount [MDP_ADF_MAXTRIPLE], the centres over the cap, the bad tags
};
// per-atom coordination numbers (coord.hip): the binning of a read and the rows it writes, one per owned atom
struct MdpCoord : MdpMeasure {
  int ncol = 0, ntypes = 0, gbit = 0;
  double cutoff = 0.0;
  DevBuf<unsigned> tab;            // [kBinTypes] per type code the columns whose range holds it
  MdpBinning bin;
  DevBuf<double> val;              // [nlocal][ncol] in the context's owned order
};
// the per-atom centro-symmetry parameter (centro.hip): the same, with the counters of a read
struct MdpCentro : MdpMeasure {
  int nnn = 0, ntypes = 0, gbit = 0;
  long long few = 0;               // centres with fewer than nnn partners at the last read
  double cutoff = 0.0;
  MdpBinning bin;
  DevBuf<double> val;              // [nlocal]
  DevBuf<unsigned long long> cnt;  // centres over the cap of the short list, centres with fewer than nnn partners, (unused) bad tags
};
// the per-atom common neighbour analysis (cna.hip): the same, with the census of a read
struct MdpCna : MdpMeasure {
  int ntypes = 0, gbit = 0;
  long long counts[6] = {0, 0, 0, 0, 0, 0}; // group atoms of pattern 0 .. 5 at the last read
  long long over = 0;              // centres with more than MDP_CNA_MAXNEAR neighbours at the last read
  double cutoff = 0.0;
  MdpBinning bin;
  DevBuf<double> val;              // [nlocal]
  DevBuf<unsigned long long> cnt;  // centres per pattern [6], centres over the cap of the short list, (unused) bad tags
};
// binned sums of m, m v and m v^2 (profile.hip): the bins and the table of a read; nothing here is read by a step, a list build,
// msd or rdf
struct MdpProfile : MdpMeasure {
  int ndim = 0, dim[3] = {0, 0, 0}, nbin[3] = {1, 1, 1}, gbit = 0;
  long long rows = 0;
  DevBuf<double> part;             // per-block maxima of |t_k|, MDP_PROFILE_W per block, then the MDP_PROFILE_W maxima
  DevBuf<unsigned long long> out;  // [rows][MDP_PROFILE_W] sums (two's complement), [rows] counts, then the column flags
};
// the heat current (heatflux.hip): nothing but the partials of a read; the tallies it reads are the run's own (eatom, vatom)
struct MdpHeatflux {
  DevBuf<double> part; // per-block partials, kHfW per block, then the kHfW sums
};
static constexpr int kHfW = 8; // sum (ke + pe) v (3), sum W.v (3), count, sum (ke + pe)
static constexpr int kMsdW = 9;// sum dx^2, dy^2, dz^2, count, sum m xu (3), sum m, atoms whose tag has no origin

// what the integrate kernels need to add the Langevin force of one step (md.hip nve_advance_kernel / nve_final_kernel)
// for NB slots: 1 (one bath) or MDP_LANGEVIN_MAXBATH (several, MdpLangevin::nbath > 1; a slot beyond nbath has bit 0 and
// is never picked); 0 is what the kernels without a Langevin force take and never read, laid out as 1.  Everything a lane
// takes from its bath is picked by unrolled selects on the bath index, never by indexing these arrays with it (no
// scratch) and never by a branch (lanes of different baths run the same code); with one slot the index is the constant 0
// and nothing is left to select.
// bit: the group bit of every bath.  One bath has none to tell apart, so it carries none: its arguments keep the 72 bytes
// that every instantiation of nve_advance_kernel finds the group arguments behind.
template <int NB> struct MdpLgvBits { int bit[NB] = {}; };
template <> struct MdpLgvBits<0> {};
template <> struct MdpLgvBits<1> {};
template <int NB> struct MdpLgvArgs : MdpLgvBits<NB> {
  static constexpr int nb = NB, slots = NB ? NB : 1;
  const int *tag = nullptr, *type = nullptr, *perm = nullptr; // owned atom i: tag[perm ? perm[i] : i], same for type
  const double *st = nullptr;   // MdpLangevin::st: bath k at st + k * kLgvWords
  const double *mean = nullptr; // some bath has zero yes: st + kLgvMean, component j of bath k's mean at [k * kLgvWords + j]
                                // (the mean of a bath without zero yes stays 0)
  double *part = nullptr;       // some bath has tally yes: NB partial sums of f_L . v per block, [bath]
  double tsqrt[slots] = {};     // sqrt(T(n)) of every bath
  unsigned seed[slots] = {};    // the Philox key of every bath ...
  unsigned lo = 0, hi = 0, phase = 0; // ... and the counter words of the step
};
static_assert(sizeof(MdpLgvArgs<0>) == 72 && sizeof(MdpLgvArgs<1>) == 72, "the group arguments of nve_advance_kernel stay where they are");

// what the MASK variants of the integrate kernels need to honour the groups (mdp_integrate_group, mdp_langevin_group);
// the variants without MASK never read it
struct MdpGroupArgs {
  const int *mask = nullptr, *perm = nullptr; // owned atom i: mask[perm ? perm[i] : i] (host mode: the host's order)
  int gbit = 0;                               // 0: every atom is advanced
  int lbit = 0;                               // 0: every advanced atom receives the Langevin force
};
__device__ __forceinline__ int mdp_group_mask(const MdpGroupArgs &M, int i) { return M.mask[M.perm ? M.perm[i] : i]; }
__device__ __forceinline__ bool mdp_group_moves(const MdpGroupArgs &M, int m) { return !M.gbit || (m & M.gbit); }
__device__ __forceinline__ bool mdp_group_lgv(const MdpGroupArgs &M, int m)
{ return mdp_group_moves(M, m) && (!M.lbit || (m & M.lbit)); }

// Philox4x32-10 (Salmon et al., SC11; the Random123 constants), in place on the counter c
__device__ __forceinline__ void mdp_philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
#pragma unroll
  for (int r = 0; r < 10; r++) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
  }
}

// the bath of an atom with mask m (the groups of the baths are disjoint: at most one bit matches); one bath: 0, unread
template <int NB> __device__ __forceinline__ int mdp_lgv_bath(const MdpLgvArgs<NB> &L, int m)
{
  int k = 0;
  if constexpr (NB > 1) {
#pragma unroll
    for (int b = 1; b < NB; b++) k = (m & L.bit[b]) ? b : k;
  }
  return k;
}
template <class T, int N> __device__ __forceinline__ T mdp_lgv_pick(const T (&a)[N], int k)
{
  T r = a[0];
#pragma unroll
  for (int b = 1; b < N; b++) r = k == b ? a[b] : r;
  return r;
}
// owned atom i of bath k: the random part gamma2 (u - 0.5) of its Langevin force (FixLangevin::post_force, fran), with
// the bath's table, T and seed
template <int NB>
__device__ __forceinline__ void mdp_lgv_random(const MdpLgvArgs<NB> &L, int i, int k, double &rx, double &ry, double &rz)
{
  const int a = L.perm ? L.perm[i] : i;
  const int t = L.type[a] & 15;
  unsigned c[4] = {(unsigned) L.tag[a], L.lo, L.hi, L.phase};
  mdp_philox4x32_10(c, mdp_lgv_pick(L.seed, k), 0u);
  const double g2 = L.st[k * kLgvWords + kLgvG2 + t] * mdp_lgv_pick(L.tsqrt, k);
  rx = g2 * (((double) c[0] + 0.5) * 0x1p-32 - 0.5);
  ry = g2 * (((double) c[1] + 0.5) * 0x1p-32 - 0.5);
  rz = g2 * (((double) c[2] + 0.5) * 0x1p-32 - 0.5);
}
// ... with velocity v: its Langevin force f_L = gamma1 v + fran (- the mean of fran where some bath has zero yes; a bath
// without it next to one with it subtracts the 0 its mean holds: the same bits)
template <int NB>
__device__ __forceinline__ void mdp_lgv_force(const MdpLgvArgs<NB> &L, int i, int k, double vx, double vy, double vz,
                                              double &lx, double &ly, double &lz)
{
  double rx, ry, rz;
  mdp_lgv_random(L, i, k, rx, ry, rz);
  const double g1 = L.st[k * kLgvWords + (L.type[L.perm ? L.perm[i] : i] & 15)];
  lx = g1 * vx + rx;
  ly = g1 * vy + ry;
  lz = g1 * vz + rz;
  if (L.mean) {
    lx -= L.mean[k * kLgvWords];
    ly -= L.mean[k * kLgvWords + 1];
    lz -= L.mean[k * kLgvWords + 2];
  }
}

// a . b of two 3-vectors with the roundings written out: the first product is rounded, the other two are fused.  Left
// to -ffp-contract=fast the compiler picks the product it rounds per kernel and per build, and the Langevin tally (a sum
// of these) would move in its last bit whenever the code around it changes.
__device__ __forceinline__ double mdp_dot3(double a0, double b0, double a1, double b1, double a2, double b2)
{ return fma(a2, b2, fma(a1, b1, a0 * b0)); }

// The fixed-order sums behind the bitwise reproducible thermostats.  The per-block sum: W values per lane of a 256-lane
// workgroup into part[W * blockIdx.x + k] -- lanes by xor-shuffle 32..1, then the four waves as (w0 + w1) + (w2 + w3).
// Every lane must call it.
template <int W> __device__ __forceinline__ void mdp_block_sum_256(const double *e, double *part)
{
  __shared__ double wsum[W][4];
#pragma unroll
  for (int k = 0; k < W; k++) {
    double s = e[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < W) part[W * (size_t) blockIdx.x + k] = (wsum[k][0] + wsum[k][1]) + (wsum[k][2] + wsum[k][3]);
}
__device__ __forceinline__ void mdp_block_sum_256(double e, double *part) { mdp_block_sum_256<1>(&e, part); }

// ... for S groups of five sums each (the heat sources, the indenters), with one difference: a wave none of whose lanes
// met an atom of group b leaves the five sums of b at the 0.0 they are, without shuffling zeros around -- the same bits,
// and what the pass costs where the groups are strips of a large box (most waves see no atom of any, the others one).
// seen: bit b set if this lane met an atom of group b; the branch is on a ballot, so a wave takes it as one.  Every lane
// must call it.
template <int S> __device__ __forceinline__ void mdp_block_sum_256_seen(const double *e, const int seen, double *part)
{
  constexpr int W = 5 * S;
  __shared__ double wsum[W][4];
#pragma unroll
  for (int b = 0; b < S; b++) {
    const bool any = __ballot((seen >> b) & 1) != 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      double s = e[5 * b + j];
      if (any)
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if ((threadIdx.x & 63) == 0) wsum[5 * b + j][threadIdx.x >> 6] = s;
    }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < W) part[W * (size_t) blockIdx.x + k] = (wsum[k][0] + wsum[k][1]) + (wsum[k][2] + wsum[k][3]);
}

// The slot sum: ONE 256-lane workgroup adds npart slots of W values, out[k] = sum over b of part[W * b + k] on every
// lane -- slots strided by 256 per lane, then the tree 128..1 in shared memory; one pass over the slots for all W.
template <int W> __device__ __forceinline__ void mdp_slot_sum_256(const double *__restrict__ part, int npart, double *out)
{
  __shared__ double red[W][256];
  double s[W] = {};
  for (int b = threadIdx.x; b < npart; b += 256)
#pragma unroll
    for (int k = 0; k < W; k++) s[k] += part[W * (size_t) b + k];
#pragma unroll
  for (int k = 0; k < W; k++) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int) threadIdx.x < h)
#pragma unroll
      for (int k = 0; k < W; k++) red[k][threadIdx.x] += red[k][threadIdx.x + h];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < W; k++) out[k] = red[k][0];
}
// ... as a kernel of its own, launched <<<1, 256>>>: out[k] = the sum of slot k (the reads of msd.hip and heatflux.hip)
template <int W>
__global__ __launch_bounds__(256) void mdp_slot_total_kernel(const double *__restrict__ part, const int npart, double *__restrict__ out)
{
  double s[W];
  mdp_slot_sum_256<W>(part, npart, s);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < W; k++) out[k] = s[k];
}

// The style-level displacement test of one atom (MdpStyleCheck), shared by the integrate kernel (owned atoms, flag words
// [0..4)) and the halo unpack (remote ghosts, [4..8)).  two_steps: the atom's way in two steps at its current speed, a
// quarter on top for its acceleration.  The triggers are read one compute late and fire early by a fixed margin that
// stands for two steps of motion (0.07 / 0.1 A: 35 / 50 A/ps at 1 fs); an atom faster than that -- the tail of a 5 000 K
// melt -- fires by its OWN two steps instead, so what it reaches before the answer is read is still inside the limit.
__device__ __forceinline__ bool mdp_reaches(const double d2, const double hardsq, const double two_steps)
{
  const double rem = sqrt(hardsq) - two_steps; // will the atom be beyond `hard` two steps on?
  return rem <= 0.0 || d2 > rem * rem;
}
struct MdpStyleVote { bool a = false, ah = false, p = false, ph = false; }; // beyond: list trigger, half the inner skin, pruning trigger, half the buffer
__device__ __forceinline__ void mdp_style_test(const MdpStyleCheck &SC, const size_t i, const double4 &x, const double two_steps,
                                               MdpStyleVote &w)
{
  auto test = [&](const mdp_hold_t *ref, const double trigsq, const double hardsq, bool &far, bool &toofar) {
    const double dx = x.x - ref[3 * i], dy = x.y - ref[3 * i + 1], dz = x.z - ref[3 * i + 2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    far = d2 > trigsq || mdp_reaches(d2, hardsq, two_steps);
    toofar = d2 > hardsq;
  };
  if (SC.xa) test(SC.xa, SC.trig_a, SC.hard_a, w.a, w.ah);
  if (SC.xp) test(SC.xp, SC.trig_p, SC.hard_p, w.p, w.ph);
}
// Every lane of the workgroup must reach the vote: the wave votes with ALL its lanes, then lane 0 stores (a vote inside
// the lane-0 branch would count lane 0 alone).  Pinned host words zeroed by the host: plain idempotent stores.
__device__ __forceinline__ void mdp_style_vote(const MdpStyleCheck &SC, const MdpStyleVote &w, const int base)
{
  if (!SC.flag) return;
  const bool wa = __any(w.a), wah = __any(w.ah), wp = __any(w.p), wph = __any(w.ph);
  if ((threadIdx.x & 63) == 0) {
    if (wa) SC.flag[base] = 1;
    if (wah) SC.flag[base + 1] = 1;
    if (wp) SC.flag[base + 2] = 1;
    if (wph) SC.flag[base + 3] = 1;
  }
}

struct mdp_ctx {
  MdpLedger ledger;                       // bytes of every DevBuf between the two scopes: mdp_device_bytes(ctx)
  MdpLedgerScope ledger_open{&ledger};    // (first and last members but for the ledger itself)
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  // ---- potentials
  bool have_rebomos = false, have_aeam = false;
  mdp_rebomos_params rebomos_host;
  RebomosDev rebomos;
  AeamDev aeam;
  DevBuf<double> aeam_frho, aeam_rhor, aeam_z2r;
  DevBuf<double4> aeam_rhor_v4, aeam_rhor_d4, aeam_z2r_v4, aeam_z2r_d4;
  DevBuf<double> aeam_pair_d8;
  DevBuf<double2> aeam_rhor_ys, aeam_z2r_ys;
  int lds_max = 0, num_cu = 0; // device limits (queried once)
  bool ptile_reported[3] = {false, false, false};
  DevBuf<int> aeam_maps;
  DevBuf<double> aeam_par_d; // cut | rdr | rdrho of the type pairs / types (AeamDev::g_*)
  DevBuf<int> aeam_par_i;    // nr | t2rhor | t2z2r | nrho | t2frho
  std::vector<double> aeam_hcut; // host copy of cut[ti*ntypes+tj] (list cutoffs, launch geometry)
  DevBuf<double> cut_tab;    // squared list cutoffs per type pair for more than MDP_AEAM_MAXT types (md.hip CutTables)

  // ---- atoms
  int nlocal = 0, nghost = 0, nall = 0, ntypes = 0;
  bool atoms_set = false;
  int map[16];
  DevBuf<double4> xq;   // x,y,z, w = element / type-1 as double
  DevBuf<double4> xq_cell; // the same in cell order (xq[cell_perm[p]]), as of the last mdp_bin_atoms
  DevBuf<double> xraw;  // staging for host x [nall][3]
  bool rebo_host_list = false;  // host mode, rebomos: candidates and LJ rows from the host's neighbor list (mdp_rebomos_host_list)
  bool host_sort = false;       // host mode, rebomos: device storage order = Hilbert order (host_perm: device -> host index)
  DevBuf<int> host_perm;
  DevBuf<double> host_stage;    // per-atom results back in host order before the download
  // host mode on one periodic rank: every ghost is an image of an owned atom.  Once the host has handed over its box
  // (mdp_set_box_host), owner (device order, in ghost_owner) and image counts (as doubles, in ghost_shift) are derived
  // from tags and positions at mdp_set_atoms_host, and the per-step upload carries the owned atoms only.
  bool host_box_set = false, host_ghosts_derived = false;
  bool host_check_armed = false; // rebomos host mode: the displacement check ran behind the last position upload
  double host_h[6] = {1, 1, 1, 0, 0, 0}; // xprd, yprd, zprd, yz, xz, xy (Domain::h)
  DevBuf<int> host_tagmap, host_inv, host_tag_dev; // tag -> owned host index; host -> device index; tags in device order
  DevBuf<double> host_img;                         // [nghost][3] image counts (ghost_shift: the Cartesian shift at the list build)
  std::vector<std::pair<const void *, size_t>> host_regs; // host arrays page-locked in place (large x arrays)
  char *h_up[MDP_UP_RING] = {};                // pinned upload staging (a ring of chunks)
  hipEvent_t ev_up[MDP_UP_RING] = {};
  hipEvent_t ev_down[MDP_DOWN_CHUNKS] = {};    // chunked force download (host mode)
  double *h_down = nullptr;     // pinned download buffer
  size_t h_down_cap = 0;
  DevBuf<int> tag, type;
  DevBuf<double> f;     // [nall][3]
  DevBuf<double> eatom; // [nall]
  DevBuf<double> vatom; // [nall][6] per-atom virial (allocated on first use)
  DevBuf<double> acc;   // [16] eng, virial[6], flags...
  DevBuf<int> flags;    // [4] overflow etc.
  double *h_pinned = nullptr; // pinned words for small results and flag words (MdpPin names the layout)
  char *h_small = nullptr;    // pinned scratch of mdp_read_small / mdp_write_small (counts, totals, flag words)
  size_t h_small_cap = 0;

  // ---- master neighbor list (CSR over nall atoms)
  bool neigh_set = false;
  double skin = 0.0;
  DevBuf<long long> nb_off; // [nall+1]
  DevBuf<int> nb;           // [total]
  long long nb_total = 0, nb_owned_total = 0;
  std::vector<long long> h_off;
  std::vector<int> h_nb;

  // ---- REBO-MoS repacked structures
  bool rebo_packed = false;
  DevBuf<int> cand_cnt, cand_off; // [nall+1]
  DevBuf<int> cand;               // REBO candidates (r <= rcmax+skin)
  int cand_total = 0;
  // Lennard-Jones cluster pair list: MDP_CLUSTER consecutive owned atoms share one union list
  DevBuf<long long> lj_off;       // [nclus+1]
  DevBuf<int> lj_cnt;             // [nclus]
  DevBuf<int> lj;                 // union neighbours (r <= rcLJmax+skin of ANY atom of the cluster)
  long long lj_total = 0;
  int nclus = 0, cluster = MDP_CLUSTER;
  // halo overlap (multi-GPU): clusters whose lists reach no remote ghost come first in cl_order
  int remote_start = 1 << 30;
  bool centre_split = false;      // REBO centres split interior / boundary (default with remote ghosts)
  int centres_early = 0;          // rebomos: which interior centre kernels mdp_rebomos_run_begin launched (launch_centres `which`)
  int overlap_mode = 0;           // this step: 0 interior work in compute_begin, 2 nothing early (blocking order), 3 rebomos:
                                  // only the lane-per-centre kernel early (MdpDomain::ov_policy; set per step by the step calls)
  DevBuf<int> cl_flag, cl_pos, cl_order;
  DevBuf<int> lj_split;           // [nclus] number of Mo entries at the head of each row
  // Lennard-Jones tile lists (default): the MDP_TILE consecutive clusters one workgroup handles share
  // the UNION of their neighbours; its coordinates are staged in LDS once per step and the cluster rows
  // hold 16-bit indices into it (lj16), so every global gather is amortised over ~7 uses
  bool lj_tiled = false;
  int ntile = 0, tile_cap = 0, tile_maxu = 0, tile_rowmax = 0; // (rowmax: most row entries of one tile, generic builder)
  int tile_maxu_in = 0, tile_rowmax_in = 0; // the same among the tiles that reach no remote ghost (aeam, bricks)
  int lj_class_base[5] = {0, 0, 0, 0, 0}; // ranges of cl_order: small / large unions (the last two are empty)
  bool lj_ordered = false;        // cl_order in use (otherwise natural order, everything in class 0)
  int tile_small = 0;             // largest union of the "small" launch classes
  DevBuf<int> tu;                 // [ntile][tile_cap] union members (atom index), Mo first then S
  DevBuf<unsigned short> tmask;   // [ntile][tile_cap] bit g: cluster g of the tile lists the member
  // dynamic pruning of the tile rows (resident mode): between two list builds the rows are re-filtered, from the
  // current positions, to the entries within window + prune_buf of a cluster atom; the kernels walk the pruned rows
  // until an atom has moved prune_buf/2 since (second trigger of moved_kernel), then they are pruned again
  DevBuf<unsigned short> lj16_in; // pruned rows, at the offsets of the rows as built
  DevBuf<int> lj_len_in, lj_split_in; // their lengths and splits
  DevBuf<mdp_hold_t> xhold_prune; // [nall][3] positions at the last pruning
  bool prune_valid = false, prune_stale = false;
  double prune_buf = 0.3;
  int prune_epoch = 0, prune_copied_epoch = -1, prunes = 0, dangerous_prunes = 0;
  int computes_since_prune = 0;
  int tile_rows_cl = 2; // atoms per row of the current tile lists
  DevBuf<int> tile_nu;            // [ntile] members of each union
  DevBuf<int> tile_flag;          // [0] a union outgrew tile_cap   [1] largest union   [2] most row entries of a tile
  DevBuf<unsigned short> lj16;    // cluster rows, indices into the tile's union
  DevBuf<int> is_center;          // [nall]
  // fix nve on the device for a host-mode context (mdp_hnve_*, the plugins' `fix nve/mdp`)
  bool hn_on = false;
  double hn_dt = 0.0, hn_dtf = 0.0, hn_ftm2v = 0.0;
  double hn_mass[16] = {};
  DevBuf<double> hn_mass_dev;
  bool hn_v_current = false;      // c->v / c->rmass match the atoms of the last mdp_set_atoms_host
  int ovf_par = 0;                // which of the two sets of pinned overflow counts (kPinOvf) this compute uses
  bool hn_deferred_check = false; // host mode + device integrator, rebomos: the style checks ride in the integrate kernel, read a compute late
  int ang_list_n = -1;            // >= 0: ang_list holds exactly the owned angular centres of the current atoms (mdp_md_build_master_list)
  bool f_prezeroed = false;       // f[0 .. nall) was cleared by the integrate kernel / image refresh of this step (aeam)
  bool f_zero_remote_due = false; // ... except the remote ghosts' part, which this step's halo unpack clears (bricks, step mode)
  bool aeam_img_fp = false;       // the embedding kernel of this compute filled fp of the periodic self-images too
  DevBuf<int> lj_fix_stamp;       // [ntile] stamp of the compute that last listed the tile for rebo_lj_cubic_kernel
  int lj_stamp = 0;
  // hot systems: the flagged pairs of the Lennard-Jones tile kernel in per-group queues (rebo_lj_tile_kernel<.., QUEUE>)
  DevBuf<unsigned short> lj_cq;   // [ntile][16 groups][2 atoms][lj_cq_cap] items
  DevBuf<int> lj_cq_cnt;          // [ntile][16][2] entries (zero between computes)
  int lj_cq_cap = 0, lj_cq_tiles = 0;
  bool lj_queue_now = false;      // this compute's tile launches took the QUEUE variant
  DevBuf<double> lj_fixtab;       // [4][12] lo hi sw lj1 lj2 lj3 lj4 rcLJmin c2 c3 - - per pair type (cubic inner spline, rare path)
  DevBuf<int> cand_stage;         // [nall][64] candidate rows at a fixed stride, written by the counting sweep of a list build
  DevBuf<int> class_list;         // [MDP_NCLASS][nall]   class = 2 * (lane-group size index) + element
  DevBuf<int> class_count;        // [MDP_NCLASS]
  DevBuf<int> pk_cand;            // per class, per centre: its first UA*G candidates, contiguous in class order
  size_t pk_base[MDP_NCLASS] = {};
  DevBuf<int> class_merged;       // per class: interior centres then boundary centres, one list (launches over both halves)
  size_t merged_base[MDP_NCLASS_HALF] = {};
  int h_class_count[MDP_NCLASS] = {};
  DevBuf<unsigned long long> amask; // [nall] bit t: candidate t currently inside rcmax
  DevBuf<int> rev;                // [cand_total] absolute reverse slot (owned rows)
  DevBuf<int> rev16;              // [nlocal][16] the first 16 of them at a fixed stride
  DevBuf<int> ovf;                // 5 x [1+nall+1]: centres handed on this step -- to the general kernel / by the lane-per-centre kernel
  int ovf_stride = 0;
  DevBuf<unsigned long long> centre_paths; // [3] waves of rebo_centre_kernel on the full-group path / on the general loops / blend trips of the former (MDP_CENTRE_COUNT=1)
  bool centre_full_now = true;    // this compute's lane-group kernels may take the full-group path (MDP_CENTRE_FULL)
  unsigned long long *centre_cnt_now = nullptr; // ... and count their waves here (null: no counting)
  int ovf3_hot[4] = {0, 0, 0, 0}; // computes left in list mode per (part, element) list of the lane-per-centre kernel
  DevBuf<mdp_hold_t> xhold_all;   // [nall][3] positions when the style lists were built
  double skin_inner = 0.0;        // the style lists' own skin (<= the host's)
  double skin_inner_auto = 1.0;   // adaptive default of it (grows when the displacement trigger fires too often)
  double skin_inner_cap = 1.0e9;  // a skin at which a candidate row outgrew the 64-bit active mask (dense systems)
  long long computes_since_build = 0;
  bool stale_rebuild = false;     // the pending rebuild was asked for by the displacement trigger
  long long style_builds = 0;     // number of style-list builds so far
  long long dangerous_builds = 0; // deferred check saw an atom beyond half the inner skin
  // fused style-level checks (MdpStyleCheck): set armed by the last integrate kernel, event of its last writer
  // The words of a set are READ one compute after they were written (mdp_sflag_collect takes the set of the step
  // before, whose event completed long ago): no host wait on the GPU in the step, on one GPU as on several.
  int sflag_set = 0;
  bool sflag_armed = false;
  bool sflag_committed[2] = {false, false}; // the set's last writer has been queued (event recorded), not yet collected
  MdpStyleCheck sflag_chk;
  MdpStyleCheckMeta sflag_meta[2];
  hipEvent_t ev_sflag[2] = {nullptr, nullptr};
  MdpNhc nhc;                      // thermostat of the integrate calls (mdp_nhc_setup)
  MdpLangevin lgv;                 // Langevin thermostat of the integrate calls (mdp_langevin_setup)
  MdpFire fire;                    // FIRE minimiser: mdp_md_advance launches its advance kernel while it is on (mdp_fire_setup)
  MdpHeat heat;                    // constant-flux heat sources behind every final half (mdp_heat_setup)
  MdpIndent indent;                // indenters in front of the kicks (mdp_indent_setup)
  MdpSpring spring;                // tether springs in front of the kicks, behind the indenters (mdp_spring_setup)
  MdpGforce gforce;                // prescribed group forces in front of the kicks, behind the springs (mdp_gforce_setup)
  // groups (mdp_md_set_mask / mdp_hnve_set_mask, mdp_integrate_group, mdp_langevin_group)
  DevBuf<int> mask;                // [nlocal] atom->mask: device order (resident; permuted and migrated with the atoms) or the host's order
  bool mask_set = false;
  int mask_n = 0;                  // owned atoms the mask covers (host mode: as of the last mdp_hnve_set_mask)
  int group_bit = 0, lgv_bit = 0;  // 0: every atom
  // image flags (mdp_md_set_image) and the mean-squared displacement measured with them (msd.hip)
  DevBuf<int> image;               // [nlocal] atom->image, LAMMPS' 32-bit imageint: device order, remapped, permuted and migrated with the atoms
  bool image_set = false;
  MdpMsd msd;
  MdpRdf rdf;                      // pair-distance histograms of the current positions (mdp_rdf_setup)
  MdpAdf adf;                      // bond-angle histograms of the current positions (mdp_adf_setup)
  MdpCoord coord;                  // per-atom coordination numbers of the current positions (mdp_coord_setup)
  MdpCentro centro;                // per-atom centro-symmetry parameters of the current positions (mdp_centro_setup)
  MdpCna cna;                      // per-atom common neighbour analysis of the current positions (mdp_cna_setup)
  MdpProfile profile;              // binned mass, momentum and kinetic energy of the current atoms (mdp_profile_setup)
  MdpHeatflux heatflux;            // partial sums of a heat-current read (mdp_heatflux_sums)
  // eflag / vflag of the last FINISHED compute while its per-atom tallies (eatom, vatom) still describe the owned atoms in
  // their current order and state; -1 after anything that starts a compute, moves the atoms or re-orders them
  int tally_eflag = -1, tally_vflag = -1;
  bool final_pending = false;      // the host deferred the final half-kick of the finished step (mdp_md_defer_final)
  bool final_deferred_seen = false; // the host uses mdp_md_defer_final at all (older hosts: with_final is authoritative)
  bool acc_prezeroed = false; // the integrate kernel reset the accumulators: the next mdp_acc_begin launches nothing
  bool check_now = false;         // positions were rewritten by the host (mdp_md_upload_x): check the lists before use
  DevBuf<double> fnbr;            // [cand_total][4] force on the slot's neighbour + its share of the pair energy
  DevBuf<double> fown;            // [nall][4] the centre's own share: -(sum of its slot forces), energy
  DevBuf<double> vslot;           // [cand_total][6] per-atom virial shares (allocated on first use)
  DevBuf<char> scan_tmp;

  // ---- AEAM work arrays
  DevBuf<double> rho, fp;         // [nall]
  DevBuf<int> ang_list;           // owned angular atoms
  DevBuf<int> ang_count;
  int h_ang_count = 0;
  int aeam_cl = 1;                // atoms per cluster of the AEAM tile lists
  bool aeam_tiled = false;        // resident mode: tile lists (tu / lj16 ...) serve the force-only steps
  bool aeam_device_lists = false; // host mode: lists built on the device from the positions (as rebomos), host list unused
  bool skin_set = false;
  bool csr_full = true;           // the CSR list holds rows for every owned atom (false: angular centres only)
  bool csr_want_full = false;     // a per-atom-virial step ran: keep building the full list
  int aeam_split = 0;             // tiles [0, aeam_split) reach no remote ghost (0: no remote ghosts / no tile lists)
  bool aeam_ang_remote = false;   // an angular centre may have a remote ghost in its row: ghost forces must travel
  int aeam_phase = 0;             // phases of the current compute already done (aeam.hip)
  int aeam_vflag = 0;             // vflag of the current compute (phase A hands it to the early three-body forces)

  // ---- binning (shared by the master-list builder and the cluster-list builder)
  MdpGrid grid;
  double bbox_lo[3] = {0, 0, 0}, bbox_hi[3] = {0, 0, 0}; // of the atoms last uploaded (host mode)

  // ---- resident MD
  bool md = false;
  mdp_md_config cfg;
  DevBuf<double> v;          // [nlocal][3]
  DevBuf<mdp_hold_t> xhold;  // [nlocal][3] positions at last build
  DevBuf<double> rmass;      // [nlocal]
  DevBuf<int> ghost_owner;   // [nghost]
  DevBuf<double> ghost_shift;// [nghost][3]
  DevBuf<double> mass_type;  // [ntypes+1] per-type masses on the device (rmass of migrated atoms)
  double h_mass[16] = {};
  MdpDomain dd;
  // binning scratch
  DevBuf<int> cell_of, cell_perm, cell_start;
  DevBuf<unsigned> sort_keys_a, sort_keys_b;
  DevBuf<int> sort_vals_b;
  DevBuf<int> nb_cnt;
  double last_eng = 0.0, last_virial[6] = {0, 0, 0, 0, 0, 0};

  // ---- timing
  bool timing = false;
  hipEvent_t ev[8] = {};
  hipEvent_t ev_sb[8] = {}, ev_se[8] = {}; // spans
  unsigned span_mask = 0;                  // spans recorded since the last mark 0 / span reset
  bool timing_spans = false;
  bool ev_made = false;
  int ev_marks = 0;
  double t_ms[8] = {};
  MdpLedgerScope ledger_close{nullptr};
};

int mdp_fail(mdp_ctx *c, int code, const char *fmt, ...);

// Layout of mdp_ctx::h_pinned, in doubles (kPinWords of them, zeroed at mdp_create).  The int words are written by kernels
// with plain stores (or by a copy) and are valid for the host once the event / stream wait named here has returned.
enum MdpPin {
  kPinAcc = 0,        // [0..9) doubles: acc[0..9) as copied by fetch_acc / aeam_fetch / mdp_md_thermo; read after their stream wait
  kPinFlags = 16,     // 5 ints: the overflow flags, copied and read with kPinAcc (mdp_flags_check)
  kPinHostCheck = 24, // 4 ints: rebomos' immediate displacement check (rebomos_check_launch -> moved_kernel); host zeroes, reads after a stream wait
  kPinMoved = 28,     // 2 ints: `check yes` of the host-level skin (mdp_moved_arm zeroes; moved_kernel / the integrate kernel write; mdp_moved_take reads behind ev_moved_ref)
  kPinSflag = 32,     // 2 sets x 8 ints: the style-level checks (mdp_sflag_arm zeroes a set; the integrate kernel writes [0..4),
                      //         the halo unpack [4..8); mdp_sflag_collect reads the other set behind ev_sflag[set])
  kPinOvf = 40,       // 2 sets x 4 ints (ovf_par): centres that outgrew the lane-per-centre kernel, per list
                      //         (rebo_centre_general_kernel writes; read two computes later, behind mdp_sflag_collect's wait)
  kPinGeneral = 44,   // 1 int: centres handed to the general kernel (same writer; statistics)
  kPinCubic = 45,     // 1 int: tiles listed for the cubic Lennard-Jones spline (the cubic / queue kernels write; sizes later grids)
  kPinGlob = 46,      // 1 int: some rank's owned atom moved (unpack_x_kernel writes; mdp_dd_comm_step_begin reads behind ev_glob_ref)
  kPinCubicWalk = 47, // 1 int: queue mode, tiles whose queues overflowed (rebo_lj_cubic_kernel writes; sizes later grids)
  kPinFire = 48,      // 3 doubles: the minimiser's stop code, iteration count and sum f.f (fire_control_kernel writes; mdp_fire_iterate
                      //         polls the stop code without waiting: it is valid once a later kernel's event has been waited for)
  kPinWords = 64
};
static_assert(kPinFire + 3 <= kPinWords, "the last pinned word must fit the allocation");
inline int *mdp_pin(const mdp_ctx *c, MdpPin word) { return (int *) (c->h_pinned + word); }

// The constants of a velocity-Verlet step, for a resident context (mdp_md_setup) and a host-linked one (mdp_hnve_setup)
struct MdpStep {
  double dt, dtf, ftm2v; // dtf = 0.5 dt ftm2v
  const double *mass;    // per-type host masses [16] (unused types: 0.0 resident, 1.0 host-linked)
};
inline MdpStep mdp_step(const mdp_ctx *c)
{
  if (c->md) return {c->cfg.dt, 0.5 * c->cfg.dt * c->cfg.ftm2v, c->cfg.ftm2v, c->h_mass};
  return {c->hn_dt, c->hn_dtf, c->hn_ftm2v, c->hn_mass};
}

// The deferred displacement triggers are read one compute late, so they fire `margin` early.  The margins were
// measured for the reference inputs' 1 fs step (0.1 A covers two steps at 50 A/ps); they scale with the time step of a
// resident run (a 5 fs step moves atoms five times as far before the answer is read).
inline double mdp_margin_scale(const mdp_ctx *c) { return c->md && c->cfg.dt > 0.001 ? c->cfg.dt / 0.001 : 1.0; }

// Small device <-> host transfers (counts, totals, flag words) go through a pinned scratch buffer of the CONTEXT and
// are complete on return: no asynchronous copy ever targets a stack variable or a std::vector (pageable memory goes
// through the runtime's shared staging path, and a host that drives several contexts from several threads must not
// depend on how that path behaves under concurrency).
struct MdpRead {
  const void *d_src;
  size_t bytes;
  void *h_dst;
};
int mdp_read_small(mdp_ctx *c, const MdpRead *r, int n);                       // waits for the stream
int mdp_read_one(mdp_ctx *c, const void *d_src, size_t bytes, void *h_dst);    // waits for the stream
int mdp_write_small(mdp_ctx *c, void *d_dst, const void *h_src, size_t bytes); // waits for the stream

#define MDP_HIP(c, call)                                                                             \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return mdp_fail((c), MDP_EHIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
  } while (0)

#define MDP_TRY(expr)                                                                                \
  do {                                                                                               \
    int rc_ = (expr);                                                                                \
    if (rc_ != MDP_OK) return rc_;                                                                   \
  } while (0)

// One kernel launch: raises the kernel's dynamic-LDS limit when `lds` needs more than the 48 KB a kernel gets unasked,
// launches, and reports a launch error through the context.  The arguments convert to the kernel's parameter types as in
// a launch written out.
template <typename... P, typename... A>
inline int mdp_launch(mdp_ctx *c, void (*kernel)(P...), int grid, int block, size_t lds, hipStream_t st, A &&...args)
{
  if (lds > 48 * 1024)
    MDP_HIP(c, hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
  kernel<<<grid, block, lds, st>>>(std::forward<A>(args)...);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

// A run-time bool as a compile-time one: f(std::true_type{}) or f(std::false_type{}), for picking a kernel's template arguments
template <class F> inline int mdp_with_bool(const bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// The tile rows the kernels walk now: the pruned copy while a pruning is valid (lengths in `len`), the rows as built
// otherwise (len null: a row's length is the distance to the next row's offset)
struct MdpRows {
  const int *len, *split;
  const unsigned short *lj16;
};
inline MdpRows mdp_rows(const mdp_ctx *c)
{
  if (c->prune_valid) return {c->lj_len_in.p, c->lj_split_in.p, c->lj16_in.p};
  return {nullptr, c->lj_split.p, c->lj16.p};
}
// new rows were built: the pruned copy is made by the next compute that wants it
inline void mdp_rows_renewed(mdp_ctx *c)
{
  c->prune_valid = false;
  c->prune_stale = false;
  c->prune_epoch++;
}

// Does aeam take tile lists (resident mode, or host mode with lists built on the device)?  MDP_AEAM_TILE=0 keeps the CSR
// kernels; the tile kernels carry the parameters of up to MDP_AEAM_MAXT types in their arguments / in LDS.  Asked by the
// master-list builder (which rows the CSR list needs) and by mdp_aeam_prepare (whether to build the tiles): one answer.
inline bool aeam_wants_tiles(const mdp_ctx *c)
{
  const char *e = getenv("MDP_AEAM_TILE");
  return (c->md || c->aeam_device_lists) && !(e && atoi(e) == 0) && c->aeam.ntypes <= MDP_AEAM_MAXT;
}

// modules
int mdp_pack_xq(mdp_ctx *c, const double *d_x3, const int *d_type_or_null, int count = -1); // xraw/type -> xq (first `count` atoms; -1: all)
int mdp_rebomos_host_precheck(mdp_ctx *c);                 // host mode: displacement check behind the position upload
int mdp_host_ghost_scalar(mdp_ctx *c, double *d_a);        // host mode, derived images: a[image] = a[owner]
int mdp_host_ghost_fold(mdp_ctx *c, int w, double *d_a);   // a[owner] += a[image], a[image] = 0 (w doubles per atom)
int mdp_hold(mdp_ctx *c, int n, mdp_hold_t *d_hold);        // d_hold = positions of the first n atoms (reference of a displacement check)
// displacement check of the first n atoms on at most max_grid blocks: flag[0] / flag[1] = some atom is beyond sqrt(trigsq) /
// sqrt(hardsq) from d_hold; with d_prune, flag[2] / flag[3] the same against d_prune.  flag: pinned host memory, zeroed by the caller
int mdp_moved(mdp_ctx *c, int n, int max_grid, double trigsq, double hardsq, const mdp_hold_t *d_hold, int *flag,
              const mdp_hold_t *d_prune = nullptr, double ptrigsq = 0.0, double phardsq = 0.0);
int mdp_scan_exclusive_int(mdp_ctx *c, const int *d_in, int *d_out, int n);  // d_out[n] = total (n+1 entries)
int mdp_chunk_by_element(mdp_ctx *c, int n, int n_owned, const int *d_idx_in, int *d_idx_out, const double4 *d_xq,
                         const int *d_type, const int *d_map); // element-sorted runs of 32 owned atoms (stable)
int mdp_scan_exclusive_i64(mdp_ctx *c, const int *d_in, long long *d_out, int n);
int mdp_rebomos_repack(mdp_ctx *c);
// keeps the pruned rows current before the kernels walk them: adapts the buffer, prunes (again) when due.  own_check: the
// style reads the displacement flags itself (rebomos); may_prune false: a pruning that is due is only reported (tiles.hip)
int mdp_prune_upkeep(mdp_ctx *c, const double cut[4], double skin, bool own_check, bool may_prune, bool *due);
// the tile rows (cl atoms per cluster; two classes of atoms: type 0 | others) within P.ljlist_cutsq, members from the bin
// grid (mdp_bin_atoms) or, from_csr, from the host's neighbor list; `ride` (may be null): a small read of the caller's
// that goes with the builder's own blocking read of the row total (made only when *ok)
int mdp_tile_rows_build(mdp_ctx *c, const RebomosDev &P, int cl, bool from_csr, const MdpRead *ride, bool *ok);
int mdp_tile_lists_build(mdp_ctx *c, const double cutsq[4], int cl, bool *ok); // ... for another two-type style (aeam), from the bin grid
int mdp_rebomos_run(mdp_ctx *c, int eflag, int vflag, bool zero_f);
int mdp_rebomos_run_begin(mdp_ctx *c, int eflag, int vflag);
int mdp_rebomos_run_end(mdp_ctx *c, int eflag, int vflag);
int mdp_aeam_prepare(mdp_ctx *c);
int mdp_aeam_run_begin(mdp_ctx *c, int eflag, int vflag);       // interior density tiles (halo in flight)
int mdp_aeam_run_density(mdp_ctx *c, int eflag);
int mdp_aeam_run_force_begin(mdp_ctx *c, int eflag, int vflag); // interior force tiles (fp / ghost forces in flight)
int mdp_aeam_run_force(mdp_ctx *c, int eflag, int vflag);
int mdp_md_build_master_list(mdp_ctx *c);
int mdp_md_build_neighbors_impl(mdp_ctx *c);
int mdp_bin_atoms(mdp_ctx *c, double cutoff, const double lo[3], const double hi[3]); // fills c->grid, cell_perm, cell_start
void mdp_time_mark(mdp_ctx *c, int k);
void mdp_span_begin(mdp_ctx *c, int k); // per-phase device time as independent (begin, end) event pairs: aeam
void mdp_span_end(mdp_ctx *c, int k);
int mdp_host_pinned_reserve(mdp_ctx *c, size_t ndoubles); // c->h_down: pinned download buffer (host mode)
int mdp_host_upload(mdp_ctx *c, void *d_dst, const void *h_src, size_t bytes); // pageable host array -> device, pipelined through pinned staging
int mdp_host_refresh_ghosts(mdp_ctx *c);                  // host mode, images kept by the library: owner + count * h of this step
int mdp_md_advance(mdp_ctx *c, bool with_final, int *flag, double trigsq, double hardsq); // integrate kernel (+ displacement check)
int mdp_md_ghost_fold(mdp_ctx *c, int w, double *d_a); // resident mode: what the periodic self-images collected (w doubles per atom) onto their owners
int mdp_md_flush_final(mdp_ctx *c); // completes a final half the host deferred (resident mode), before anything that needs full-step velocities
// `neigh_modify check yes` of the host-level skin, one step late (kPinMoved).  _take: the answer of the check the previous
// call queued (waits for its event; 0 if none is pending); _arm: zeroes the words, gives the squared limits for `skin`;
// _post: the event behind the kernel that writes the words (borrow_sflag: the style-check event the caller committed there)
int mdp_moved_take(mdp_ctx *c, int *moved, int *dangerous);
int *mdp_moved_arm(mdp_ctx *c, double skin, double *trigsq, double *hardsq);
int mdp_moved_post(mdp_ctx *c, bool borrow_sflag);
// thermostat (nhc.hip), around the integrate kernels when c->nhc.on.  _open: before the kernel of an initial half (fused
// with the pending final half if with_final): the chain update(s) of the step; *vscale = the device word the integrate
// kernel scales the velocities by.  _final: a final half on its own (kick, chain update, velocity scaling).
int mdp_nhc_open(mdp_ctx *c, bool with_final, const double **vscale);
int mdp_nhc_final(mdp_ctx *c);
// Langevin thermostat (langevin.hip), around the integrate kernels when c->lgv.on.  _open: before a kernel that
// first consumes a compute's forces (the fused final + initial, the setup step's initial half, a final half on its own):
// *apply = whether this kernel adds the force; if so *L is filled (and the zero pre-pass queued).  Advances the step
// counter when `initial`.  _close: behind that kernel (the tally of the step).  NB: 1 with one bath on,
// MDP_LANGEVIN_MAXBATH with several (c->lgv.many()); langevin.hip instantiates these two.
template <int NB> int mdp_lgv_open(mdp_ctx *c, bool with_final, bool initial, bool *apply, MdpLgvArgs<NB> *L);
template <int NB> int mdp_lgv_close(mdp_ctx *c, const MdpLgvArgs<NB> &L);
// groups: *masked = whether the integrate calls take the MASK variants now (a group bit is set), *M filled if so; fails
// with MDP_ESTATE when a group is set and no mask covers the current atoms
int mdp_group_args(mdp_ctx *c, bool *masked, MdpGroupArgs *M);
// several baths and a mask: count the atoms in more than one bath, once per mask or bath set-up, and refuse any
int mdp_lgv_check_disjoint(mdp_ctx *c, const char *who);
// heat sources (heat.hip) when c->heat.on.  _pass: behind a plain final half that completes a step: the sums, the control
// workgroup and the rescaling of the sources that are due at that step (nothing when none is).  _count_step: an initial
// half begins the next step.  _mask: a mask was uploaded (counts it again).  _check: behind a stream wait: the latched
// error, as MDP_ESTATE
int mdp_heat_pass(mdp_ctx *c);
inline void mdp_heat_count_step(mdp_ctx *c)
{
  if (!c->heat.on) return;
  c->heat.step++;
  c->heat.started = true;
}
int mdp_heat_mask(mdp_ctx *c, const char *who);
int mdp_heat_check(mdp_ctx *c);
// prescribed group forces (gforce.hip) when c->gforce.on: a mask was uploaded (counts the AVE sharing rule again)
int mdp_gforce_mask(mdp_ctx *c, const char *who);
// The post-force stages of a context, in the order their passes run (between the first two the order only affects the
// rounding of f; the group forces come last because setforce and aveforce overwrite what is there).  base: the
// stage's MdpPostForce; pass: its kernels for the forces the context holds, which are those of step first + nhalf
// (indent.hip, spring.hip, gforce.hip); api, many, one: the nouns of its messages.  The rule they share stands here and in
// postforce.hip alone: a pass runs exactly once for the forces the context holds, in front of the kick that first consumes
// them or of a state read, and a stage's pass never runs before the passes of the stages in front of it that are due.
int mdp_indent_pass(mdp_ctx *c);
int mdp_spring_pass(mdp_ctx *c);
int mdp_gforce_pass(mdp_ctx *c);
enum MdpStageId { kStageIndent = 0, kStageSpring, kStageGforce, kStageCount };
struct MdpStage {
  MdpPostForce &(*base)(mdp_ctx *);
  int (*pass)(mdp_ctx *);
  const char *api, *many, *one;
};
inline constexpr MdpStage kMdpStages[kStageCount] = {
    {[](mdp_ctx *c) -> MdpPostForce & { return c->indent; }, mdp_indent_pass, "mdp_indent", "indenters", "indenter"},
    {[](mdp_ctx *c) -> MdpPostForce & { return c->spring; }, mdp_spring_pass, "mdp_spring", "springs", "spring"},
    {[](mdp_ctx *c) -> MdpPostForce & { return c->gforce; }, mdp_gforce_pass, "mdp_gforce", "group forces", "group force"},
};
// brings the forces the context holds up to date through stage `through`: the passes that are on and not `applied`, in
// list order.  md_final_half and md_launch_advance (md.hip) call it first thing, for all stages
inline int mdp_postforce_apply(mdp_ctx *c, int through = kStageCount - 1)
{
  for (int s = 0; s <= through; s++) {
    MdpPostForce &h = kMdpStages[s].base(c);
    if (!h.on || h.applied) continue;
    MDP_TRY(kMdpStages[s].pass(c));
    h.applied = true;
  }
  return MDP_OK;
}
// behind an initial half: the atoms have moved, a compute follows and overwrites f
inline void mdp_postforce_count_step(mdp_ctx *c)
{
  for (const MdpStage &s : kMdpStages) {
    MdpPostForce &h = s.base(c);
    if (!h.on) continue;
    h.nhalf++;
    h.applied = false;
  }
}
// the life cycle the stages share (postforce.hip); the four entry points of a kind bring their own argument checks.
// _refuse_setup: what no stage's _setup goes with.  _commit: behind the last refusal of a _setup -- completes a deferred
// final half with the stage off, zeroes st (`words` doubles), stores n, the bits and the n configurations (cfg_bytes each)
// and restarts the stage at step 0, on.  _run, _state, _off: the entry points of those names behind their null checks.
// _release: frees what stage s holds ahead of the context's end (_off).  mdp_refuse_if_on: the first stage that is on refuses `who`
enum MdpRefuse { kRefuseOffFirst, kRefuseOneRank };
int mdp_postforce_refuse_setup(mdp_ctx *c, int s);
int mdp_postforce_commit(mdp_ctx *c, int s, int words, int n, const int *groupbit, void *cfg_dst, const void *cfg, size_t cfg_bytes);
int mdp_postforce_run(mdp_ctx *c, int s, long long first);
int mdp_postforce_state(mdp_ctx *c, int s, int k, int len, double *out);
int mdp_postforce_off(mdp_ctx *c, int s);
void mdp_postforce_release(mdp_ctx *c, int s);
int mdp_refuse_if_on(mdp_ctx *c, const char *who, MdpRefuse how);
// groups: whether the mask covers the current atoms, and the mask in the host's order (host mode) for a kernel that reads
// it through mdp_group_mask alone (no group bits)
inline bool mdp_mask_current(const mdp_ctx *c) { return c->mask_set && c->mask_n == c->nlocal; }
inline MdpGroupArgs mdp_mask_args(const mdp_ctx *c)
{
  MdpGroupArgs M;
  M.mask = c->mask.p;
  M.perm = !c->md && c->host_sort ? c->host_perm.p : nullptr; // host mode: the mask is in the host's order
  return M;
}
// the group bits of the n slots that are on (a bit of 0: every owned atom; a slot beyond n is never looked at) and
// whether any is set: the mask is read.  Bits: MdpSlotBits, or a kernel's own argument type derived from it
struct MdpSlotBits {
  int n = 0;
  int bit[kStageSlots] = {0, 0, 0, 0};
  int any = 0;
};
template <class Bits = MdpSlotBits> Bits mdp_slot_bits(int n, const int *bit)
{
  Bits B;
  B.n = n;
  for (int k = 0; k < n; k++) {
    B.bit[k] = bit[k];
    B.any |= bit[k];
  }
  return B;
}
// measure_bin.hip, queued on the stream: a grid with cells >= cutoff / 2 over the padded hull of the brick (stencil: 2 cells each
// way), every owned and ghost atom sorted into it, b.cell_start and the cell-ordered records b.rec = {x, y, z, code} with
// code = (member ? type : 0) | (owned ? kBinOwned : 0).  member: by tag - 1 over 1 .. ntag, or nullptr for every atom; an atom
// whose tag has no entry counts in *d_bad and is no member.  Needs nall > 0.
int mdp_measure_bin(mdp_ctx *c, MdpBinning &b, double cutoff, int ntypes, int ntag, const unsigned char *d_member,
                    unsigned long long *d_bad, MdpGrid &g);
// what a setup or a read of such a measurement needs: a resident context with mdp_dd_setup, on its device
int mdp_measure_require(mdp_ctx *c, const char *who);
// the workgroups of a measurement kernel that strides over nchunk chunks (the histograms of rdf.hip and adf.hip, the range and
// the sums of profile.hip): min(nchunk, resident), and no more than the test hook MDP_MEASURE_GRID when that is a positive
// integer (read at every read; the sums are integers and the range is a maximum, so any value reads the same)
int mdp_measure_grid(int nchunk, int resident);
// ... and `resident` for a kernel of 256 lanes with lds_bytes of LDS per workgroup: as many workgroups as the LDS of a CU (160 KB)
// holds of them, 8 at the most (32 waves per CU), on every CU
int mdp_measure_resident(mdp_ctx *c, size_t lds_bytes, int &resident);
// What the setups of the neighbour measurements (rdf, adf, coord, centro) share.  The atom types of the run, 1 .. 15:
int mdp_measure_ntypes(mdp_ctx *c, const char *who, int &ntypes);
// the n type bounds lo, hi, lo, hi, ... of the index-th (from 1) `noun` (pair, triple, column) lie in 1 .. ntypes, and no lo > hi
int mdp_measure_type_ranges(mdp_ctx *c, const char *who, const char *noun, int index, int ntypes, int n, const int *lohi);
// The ghost shell is as of the last reneighbouring and cutghost wide; two atoms have since approached by up to half a skin
// each, so only the partners within cutghost - skin are all present: mdp_measure_shell_limit (an allowance of 1e-12 for a
// limit the caller formed as cutghost - skin is the checks').  At setup: `what` (a cutoff, an outer radius) of r reaches `whom`
// (pairs, neighbours, partners) inside it; at a read: the `what` of `setup` (its name for the message) still does.
inline double mdp_measure_shell_limit(const mdp_ctx *c) { return c->dd.cutghost - c->cfg.skin; }
int mdp_measure_shell_setup(mdp_ctx *c, const char *who, const char *what, const char *whom, double r);
int mdp_measure_shell_read(mdp_ctx *c, const char *who, const char *what, double r, const char *setup);
// the member table of a histogram setup by tag - 1 (or nullptr: everyone) goes to the device, and the caller's array is free
// on return; ntag_kept: ntag, or 0 without a table
int mdp_measure_member(mdp_ctx *c, const char *who, int ntag, const unsigned char *member_by_tag, DevBuf<unsigned char> &d_member,
                       int &ntag_kept);
// A histogram read (rdf.hip, adf.hip) before it bins: `what` of the setup still lies inside the ghost shell, a final half the
// host deferred is completed as every blocking read completes it (positions are read; the integrate kernel of the step is
// ahead on the stream), and the nout words of out are zeroed ...
int mdp_hist_open(mdp_ctx *c, const char *who, const char *what, double r, const char *setup, unsigned long long *d_out, int nout);
// ... and after its kernel: the words on the host; the last one counts the atoms whose tag the member table does not hold
int mdp_hist_download(mdp_ctx *c, const char *who, const char *setup, const unsigned long long *d_out, int nout, int ntag,
                      std::vector<unsigned long long> &host);
// the end of an mdp_{msd,rdf,profile}_setup: the measurement is on, under a serial that is new in this process (one
// counter for all kinds and contexts: unique per setup, and growing)
inline void mdp_measure_start(MdpMeasure &h)
{
  static std::atomic<long long> serial{0};
  h.serial = ++serial;
  h.on = true;
}
// the four words of mdp_*_info: on, two words of the kind's own, the serial; all 0 while off
inline int mdp_measure_info(const MdpMeasure &h, const long long a, const long long b, long long out[4])
{
  out[0] = h.on ? 1 : 0;
  out[1] = h.on ? a : 0;
  out[2] = h.on ? b : 0;
  out[3] = h.on ? h.serial : 0;
  return MDP_OK;
}
// mdp_*_off: `release` is the kind's own (file-local): its buffers go now, not with the context
inline int mdp_measure_off(mdp_ctx *c, void (*release)(mdp_ctx *))
{
  if (!c) return MDP_EINVAL;
  MDP_HIP(c, hipSetDevice(c->device));
  release(c);
  return MDP_OK;
}
// a read or a setup over a group: a mask is there, and (need_current) it covers the atoms as they are now
inline int mdp_require_group_mask(mdp_ctx *c, const char *who, const int gbit, const bool need_current)
{
  if (gbit && (!c->mask_set || (need_current && c->mask_n != c->nlocal)))
    return mdp_fail(c, MDP_ESTATE, "%s: a group is set but no mask covers the current atoms (mdp_md_set_mask)", who);
  return MDP_OK;
}
// What a per-atom read (coord.hip, centro.hip) checks before it bins: the cutoff of its setup still lies inside the ghost
// shell, and the mask covers the atoms; then the final half a host deferred is completed, as before every blocking read.
inline int mdp_peratom_open(mdp_ctx *c, const char *who, const double cutoff, const int gbit)
{
  MDP_TRY(mdp_measure_shell_read(c, who, "cutoff", cutoff, "the setup"));
  MDP_TRY(mdp_require_group_mask(c, who, gbit, true));
  return mdp_md_flush_final(c);
}
// ... and what it hands over: the w values per owned atom and the owned atoms' tags, in the context's owned order
inline int mdp_peratom_download(mdp_ctx *c, const double *d_val, const int w, int *tag, double *values)
{
  const size_t n = (size_t) c->nlocal;
  if (n) {
    MDP_HIP(c, hipMemcpyAsync(values, d_val, sizeof(double) * n * w, hipMemcpyDeviceToHost, c->stream));
    MDP_HIP(c, hipMemcpyAsync(tag, c->tag.p, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  }
  MDP_HIP(c, hipStreamSynchronize(c->stream));
  return MDP_OK;
}
// the per-atom tallies are stale from here on (a compute starts, the atoms move, are re-ordered or replaced)
inline void mdp_tally_drop(mdp_ctx *c) { c->tally_eflag = c->tally_vflag = -1; }
// FIRE minimiser (fire.hip), in place of the integrate kernel when c->fire.on: the half step back / zeroing and the Euler
// step of the iteration whose control kernel was queued last, with the same votes, accumulator reset and force clear
int mdp_fire_launch_advance(mdp_ctx *c, int *flag, double trigsq, double hardsq, const MdpStyleCheck &sc, bool zero_f);
void mdp_host_add(double *dst, const double *src, size_t n); // dst += src, threaded for large arrays
int mdp_host_download_add(mdp_ctx *c, double *h_dst, double *h_stage, const double *d_src, size_t n); // chunked D2H + add
int mdp_to_host_order(mdp_ctx *c, int n, int w, const double *d_src, double *d_dst);   // per-atom arrays, device -> host order
int mdp_to_device_order(mdp_ctx *c, int n, int w, const double *d_src, double *d_dst); // host -> device order
int mdp_acc_begin(mdp_ctx *c, bool any); // zero acc (+ slots when any energy/virial is tallied)
void mdp_sflag_arm(mdp_ctx *c, MdpStyleCheck &sc);  // before the integrate kernel: which references, which flag set
int mdp_sflag_commit(mdp_ctx *c);                   // behind the last kernel that writes this step's flag words
void mdp_sflag_drop(mdp_ctx *c);                    // positions were rewritten outside the integrator: flag words in flight say nothing
int mdp_sflag_collect(mdp_ctx *c, bool *far, bool *toofar); // flags of the previous step (waits for their event): style part returned, pruning part applied
int mdp_acc_end(mdp_ctx *c, bool any);   // fold the slots into acc[0..6]
int mdp_flags_check(mdp_ctx *c, const int *hflags5); // overflow bits (last compute | sticky) -> MDP_EOVERFLOW
