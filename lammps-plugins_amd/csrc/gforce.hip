// Prescribed forces on groups, on the device: LAMMPS fix setforce, fix addforce and fix aveforce with constant values
// (FixSetForce / FixAddForce / FixAveForce::post_force), in front of every kick that first consumes a compute's forces.
// The slots act in order k = 0 .. n - 1 on one atom's force, as the fixes do in the order of their definition; with g the
// atom's force as the slots before k left it, f the slot's values and use[d] == 0 LAMMPS' NULL
//   SET:  F_k += g;                                              then g[d] = f[d] where use[d]
//   ADD:  F_k += g,  E_k -= f . xu  (xu = x + h . image, mdp_unwrap);  then g += f
//   AVE:  F_k += g,  N_k += 1;              then g[d] = F_k[d] / N_k + f[d] where use[d], the sums over the whole group
// Only AVE needs a sum over the group before an atom's later force is known, and the set-up refuses a slot that shares
// atoms with an AVE slot in front of it: so SET and ADD are local, at most one AVE is among an atom's slots and it is the
// last of them, and a lane walks its atom's slots in one go on a running force in registers (gforce_walk).  In three
// launches: per block and slot the sums of F_k and E_k and the atom counts in fixed slots (gforce_sums_kernel); one
// workgroup that adds the slots in a fixed order and leaves the state words and, for AVE slots, the value to write in
// device memory (gforce_control_kernel); one lane per owned atom that walks again and writes f (gforce_apply_kernel).  With
// no AVE slot on, what the walk of the sums kernel ends with is the atom's final force: it writes f itself
// (gforce_sums_kernel<true>) and the pass is two launches.  No float atomics and no host wait: a run is bitwise
// reproducible.  The group forces are the third post-force stage of a context, behind the indenters and the springs
// (kMdpStages, mdp_common.h): mdp_postforce_apply calls mdp_gforce_pass, and postforce.hip holds the life cycle they share.
#include "mdp_common.h"

#include <cmath>

namespace {

constexpr int kN = MDP_GFORCE_MAX;
constexpr int kLen = MDP_GFORCE_STATE_LEN;
constexpr int kGfVal = 6; // state words [6..9): the value a slot writes or adds per dimension

// everything the kernels need of the slots, by value: uniform over the grid, so it stays in scalar registers
struct GforceArgs : MdpSlotBits {
  int kind[kN] = {0, 0, 0, 0};
  int use[kN] = {0, 0, 0, 0}; // bit d: dimension d takes part
  double f[kN][3] = {};
  int add = 0;                // an ADD slot is on: positions and image flags are read
  int ave = 0;                // an AVE slot is on: the apply kernel writes f
};

__device__ __forceinline__ int gforce_in(const GforceArgs &A, const int w)
{
  int in = 0;
#pragma unroll
  for (int k = 0; k < kN; k++)
    if (k < A.n && (!A.bit[k] || (w & A.bit[k]))) in |= 1 << k;
  return in;
}

// One atom's slots in order on its running force g.  SUMS: e[5 k ..] gains g as slot k finds it and, for ADD, the energy
// (plain adds and mdp_dot3: the same roundings in every build); an AVE slot is left as it is found -- no slot behind it
// holds this atom.  Otherwise: val + kLen k holds what AVE slot k writes (gforce_control_kernel)
template <bool SUMS>
__device__ __forceinline__ void gforce_walk(const GforceArgs &A, const int in, double g[3], const double *xu, double *e,
                                            const double *__restrict__ val)
{
#pragma unroll
  for (int k = 0; k < kN; k++) {
    if (!((in >> k) & 1)) continue;
    if (SUMS) {
      e[5 * k] += g[0];
      e[5 * k + 1] += g[1];
      e[5 * k + 2] += g[2];
    }
    const int kind = A.kind[k];
    if (kind == MDP_GFORCE_ADD) {
      if (SUMS) e[5 * k + 3] -= mdp_dot3(A.f[k][0], xu[0], A.f[k][1], xu[1], A.f[k][2], xu[2]);
#pragma unroll
      for (int d = 0; d < 3; d++) g[d] += A.f[k][d];
    } else if (kind == MDP_GFORCE_SET) {
#pragma unroll
      for (int d = 0; d < 3; d++) g[d] = (A.use[k] >> d) & 1 ? A.f[k][d] : g[d];
    } else if (!SUMS) {
#pragma unroll
      for (int d = 0; d < 3; d++) g[d] = (A.use[k] >> d) & 1 ? val[k * kLen + d] : g[d];
    }
  }
}

// part[kGfW b + 5 k + j]: the sums over block b of slot k's fx, fy, fz as the slot finds them, its energy and a spare 0;
// cnt[kN b + k]: the number of its atoms.  A block takes kGfPer x 256 consecutive atoms, a lane kGfPer of them at a stride
// of 256 (coalesced), added in that order -- the per-lane layout of spring_sums_kernel.  Every lane reaches the block sum; a
// block with no atom of any slot writes zeros.  The counts are integers: a wave adds its ballots' bit counts in LDS.
// WRITE (no AVE slot is on): the walk's result is the atom's force, written here; an atom in no slot is neither read nor
// written
constexpr int kGfPer = 4;
template <bool WRITE>
__global__ __launch_bounds__(256) void gforce_sums_kernel(const int n, const double4 *__restrict__ xq, const int *__restrict__ image,
                                                          double *__restrict__ f, const GforceArgs A, const DdGeom G,
                                                          const MdpGroupArgs M, double *__restrict__ part, int *__restrict__ cnt)
{
  __shared__ int wcnt[kN];
  if (threadIdx.x < kN) wcnt[threadIdx.x] = 0;
  __syncthreads();
  double e[kGfW];
#pragma unroll
  for (int q = 0; q < kGfW; q++) e[q] = 0.0;
  int seen = 0;
#pragma unroll
  for (int j = 0; j < kGfPer; j++) {
    const int i = (blockIdx.x * kGfPer + j) * 256 + threadIdx.x;
    const int in = i < n ? gforce_in(A, A.any ? mdp_group_mask(M, i) : 0) : 0;
#pragma unroll
    for (int k = 0; k < kN; k++) { // (every lane votes: the ballot is the wave's)
      const int c = __popcll(__ballot((in >> k) & 1));
      if (c && (threadIdx.x & 63) == 0) atomicAdd(&wcnt[k], c);
    }
    if (!in) continue;
    seen |= in;
    double xu[3] = {0.0, 0.0, 0.0};
    if (A.add) mdp_unwrap(G, xq[i], image[i], xu);
    double g[3] = {f[3 * (size_t) i], f[3 * (size_t) i + 1], f[3 * (size_t) i + 2]};
    gforce_walk<true>(A, in, g, xu, e, nullptr);
    if (WRITE) {
      f[3 * (size_t) i] = g[0];
      f[3 * (size_t) i + 1] = g[1];
      f[3 * (size_t) i + 2] = g[2];
    }
  }
  mdp_block_sum_256_seen<kN>(e, seen, part);
  if (threadIdx.x < kN) cnt[kN * (size_t) blockIdx.x + threadIdx.x] = wcnt[threadIdx.x]; // (behind the block sum's barrier)
}

struct GforceCtl {
  int n = 0;
  double step = 0.0;
  int kind[kN], use[kN];
  double f[kN][3];
};

// one workgroup: the fixed-order sums, then lane 0 leaves the state words of every slot that is on; words [6..9) of an AVE
// slot are what the apply kernel writes
__global__ __launch_bounds__(256) void gforce_control_kernel(const double *__restrict__ part, const int *__restrict__ cnt,
                                                             const int npart, const GforceCtl a, double *__restrict__ st)
{
  __shared__ int atoms[kN];
  if (threadIdx.x < kN) atoms[threadIdx.x] = 0;
  __syncthreads();
  int mine[kN] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < npart; b += 256)
#pragma unroll
    for (int k = 0; k < kN; k++) mine[k] += cnt[kN * (size_t) b + k];
#pragma unroll
  for (int k = 0; k < kN; k++)
    if (mine[k]) atomicAdd(&atoms[k], mine[k]); // (integers: any order gives the same count)
  double s[kGfW];
  mdp_slot_sum_256<kGfW>(part, npart, s); // (its barriers stand between the atomics above and lane 0's reads below)
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < kN; k++) {
    if (k >= a.n) continue;
    const int na = atoms[k];
    double *w = st + k * kLen;
    w[0] = s[5 * k + 3];
    w[1] = s[5 * k];
    w[2] = s[5 * k + 1];
    w[3] = s[5 * k + 2];
    w[4] = (double) na;
    w[5] = a.step;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const bool use = (a.use[k] >> d) & 1;
      double v = use ? a.f[k][d] : 0.0;
      if (a.kind[k] == MDP_GFORCE_AVE) v = use && na ? s[5 * k + d] / (double) na + a.f[k][d] : 0.0; // (no atoms: nothing happens)
      w[kGfVal + d] = v;
    }
    w[9] += 1.0;
  }
}

// one lane per owned atom: the walk again, with the AVE values of the control kernel, and the result into f; an atom in no
// slot is neither read nor written
__global__ __launch_bounds__(256) void gforce_apply_kernel(const int n, double *__restrict__ f, const GforceArgs A, const MdpGroupArgs M,
                                                           const double *__restrict__ st)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int in = gforce_in(A, A.any ? mdp_group_mask(M, i) : 0);
  if (!in) return;
  double g[3] = {f[3 * (size_t) i], f[3 * (size_t) i + 1], f[3 * (size_t) i + 2]};
  gforce_walk<false>(A, in, g, nullptr, nullptr, st + kGfVal);
  f[3 * (size_t) i] = g[0];
  f[3 * (size_t) i + 1] = g[1];
  f[3 * (size_t) i + 2] = g[2];
}

// the counts of a set-up or a mask upload over the mask as it was handed in (any order): [k] atoms of slot k,
// [kN + kN j + k] atoms of slot k that are also in the AVE slot j in front of it
__global__ void gforce_count_kernel(const int n, const int *__restrict__ mask, const GforceArgs A, int *__restrict__ count)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int in = gforce_in(A, A.any ? mask[i] : 0);
#pragma unroll
  for (int k = 0; k < kN; k++) {
    if (!((in >> k) & 1)) continue;
    atomicAdd(count + k, 1);
#pragma unroll
    for (int j = 0; j < k; j++)
      if (((in >> j) & 1) && A.kind[j] == MDP_GFORCE_AVE) atomicAdd(count + kN + kN * j + k, 1);
  }
}

GforceArgs gforce_args(int n, const int *bit, const mdp_gforce_config *cfg)
{
  GforceArgs A = mdp_slot_bits<GforceArgs>(n, bit);
  for (int k = 0; k < n; k++) {
    A.kind[k] = cfg[k].kind;
    for (int d = 0; d < 3; d++) {
      const bool use = cfg[k].kind == MDP_GFORCE_ADD || cfg[k].use[d];
      A.use[k] |= use ? 1 << d : 0;
      A.f[k][d] = use ? cfg[k].f[d] : 0.0;
    }
    A.add |= cfg[k].kind == MDP_GFORCE_ADD;
    A.ave |= cfg[k].kind == MDP_GFORCE_AVE;
  }
  return A;
}

int gforce_no_mask(mdp_ctx *c, const char *who)
{
  return mdp_fail(c, MDP_ESTATE, "%s: a group force acts on a group but no mask covers the current atoms (%s)", who,
                  c->md ? "mdp_md_set_mask" : "mdp_hnve_set_mask after mdp_set_atoms_host");
}

// counts the current atoms for the slots of A (reads only) and refuses a slot that shares atoms with an AVE slot in front
// of it; empty: a slot without atoms is refused too (the set-up).  who: the call
int gforce_count(mdp_ctx *c, const char *who, const GforceArgs &A, bool empty)
{
  MdpGforce &h = c->gforce;
  constexpr int kC = kN + kN * kN;
  MDP_HIP(c, h.count.reserve(kC));
  const int zero[kC] = {};
  MDP_TRY(mdp_write_small(c, h.count.p, zero, sizeof zero));
  const int n = c->nlocal;
  if (n) gforce_count_kernel<<<nblk(n), 256, 0, c->stream>>>(n, c->mask.p, A, h.count.p);
  MDP_HIP(c, hipGetLastError());
  int cnt[kC];
  MDP_TRY(mdp_read_one(c, h.count.p, sizeof cnt, cnt));
  for (int k = 0; k < A.n; k++) {
    if (empty && !cnt[k]) return mdp_fail(c, MDP_ESTATE, "%s: group force %d has no atoms (group bit %d)", who, k, A.bit[k]);
    for (int j = 0; j < k; j++)
      if (cnt[kN + kN * j + k])
        return mdp_fail(c, MDP_ESTATE,
                        "%s: %d atoms of group force %d are also in group force %d, an aveforce in front of it (mdp_gforce_setup); "
                        "what follows an aveforce must not share atoms with it",
                        who, cnt[kN + kN * j + k], k, j);
  }
  return MDP_OK;
}

} // namespace

int mdp_gforce_mask(mdp_ctx *c, const char *who)
{
  MdpGforce &h = c->gforce;
  if (!h.on) return MDP_OK;
  h.counted = false;
  if (!mdp_mask_current(c)) return MDP_OK; // (the mask was withdrawn: the next pass says so)
  MDP_TRY(gforce_count(c, who, gforce_args(h.n, h.bit, h.cfg), false));
  h.counted = true;
  return MDP_OK;
}

int mdp_gforce_pass(mdp_ctx *c)
{
  MdpGforce &h = c->gforce;
  const GforceArgs A = gforce_args(h.n, h.bit, h.cfg);
  if (A.any && !mdp_mask_current(c)) return gforce_no_mask(c, "integrate");
  if (A.add && !(c->md && c->dd.on)) return mdp_fail(c, MDP_ESTATE, "group forces are on (mdp_gforce_setup) but the context has no box any more");
  if (A.add && !c->image_set)
    return mdp_fail(c, MDP_ESTATE, "group forces are on (mdp_gforce_setup) but the image flags were withdrawn (mdp_md_set_image)");
  if (A.any && !h.counted) { // (a mask upload that was refused, or a mask that came back: counted once, here)
    MDP_TRY(gforce_count(c, "integrate", A, false));
    h.counted = true;
  }
  const int n = c->nlocal, nb = nblk(n), nbs = nblk(n, 256 * kGfPer);
  MDP_HIP(c, h.part.reserve((size_t) kGfW * (nbs ? nbs : 1)));
  MDP_HIP(c, h.cpart.reserve((size_t) kN * (nbs ? nbs : 1)));
  GforceCtl a;
  a.n = h.n;
  a.step = (double) (h.first + h.nhalf);
  for (int k = 0; k < kN; k++) {
    a.kind[k] = A.kind[k];
    a.use[k] = A.use[k];
    for (int d = 0; d < 3; d++) a.f[k][d] = A.f[k][d];
  }
  const MdpGroupArgs M = A.any ? mdp_mask_args(c) : MdpGroupArgs();
  const DdGeom G = A.add ? c->dd.G : DdGeom();
  const double4 *xq = A.add ? c->xq.p : nullptr;
  const int *image = A.add ? c->image.p : nullptr;
  if (n && A.ave) gforce_sums_kernel<false><<<nbs, 256, 0, c->stream>>>(n, xq, image, c->f.p, A, G, M, h.part.p, h.cpart.p);
  if (n && !A.ave) gforce_sums_kernel<true><<<nbs, 256, 0, c->stream>>>(n, xq, image, c->f.p, A, G, M, h.part.p, h.cpart.p);
  gforce_control_kernel<<<1, 256, 0, c->stream>>>(h.part.p, h.cpart.p, nbs, a, h.st.p);
  if (n && A.ave) gforce_apply_kernel<<<nb, 256, 0, c->stream>>>(n, c->f.p, A, M, h.st.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

extern "C" {

int mdp_gforce_setup(mdp_ctx *c, int n, const mdp_gforce_config *cfg, const int *groupbit)
{
  if (!c || !cfg || !groupbit) return MDP_EINVAL;
  if (n < 1 || n > kN) return mdp_fail(c, MDP_EINVAL, "mdp_gforce_setup: %d group forces; a context takes 1 to %d", n, kN);
  bool add = false;
  for (int k = 0; k < n; k++) {
    const mdp_gforce_config &q = cfg[k];
    if (q.kind < MDP_GFORCE_SET || q.kind > MDP_GFORCE_AVE)
      return mdp_fail(c, MDP_EINVAL, "mdp_gforce_setup: group force %d: kind %d is none of set (0), add (1), ave (2)", k, q.kind);
    for (int d = 0; d < 3; d++) {
      if (q.kind == MDP_GFORCE_ADD && !q.use[d])
        return mdp_fail(c, MDP_EINVAL, "mdp_gforce_setup: group force %d: an addforce takes all three dimensions (use[%d] is 0)", k, d);
      if (q.use[d] && !std::isfinite(q.f[d])) return mdp_fail(c, MDP_EINVAL, "mdp_gforce_setup: group force %d: f[%d] must be finite", k, d);
    }
    add |= q.kind == MDP_GFORCE_ADD;
  }
  MDP_TRY(mdp_postforce_refuse_setup(c, kStageGforce));
  if (!c->md && !c->hn_on) return mdp_fail(c, MDP_ESTATE, "mdp_gforce_setup: no integrator on the context (mdp_md_setup or mdp_hnve_setup)");
  if (add) { // the energy of an addforce is taken over the unwrapped positions
    if (!c->md)
      return mdp_fail(c, MDP_ESTATE, "mdp_gforce_setup: an addforce needs a resident context (mdp_md_setup): on a host-linked one the host keeps the image flags");
    if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "mdp_gforce_setup: mdp_dd_setup not called (an addforce's unwrapped positions need the box of the brick)");
    if (!c->image_set) return mdp_fail(c, MDP_ESTATE, "mdp_gforce_setup: an addforce is among the group forces and no image is set (mdp_md_set_image)");
  }
  const GforceArgs A = gforce_args(n, groupbit, cfg);
  if (A.any && !mdp_mask_current(c)) return gforce_no_mask(c, "mdp_gforce_setup");
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(gforce_count(c, "mdp_gforce_setup", A, true));
  // (everything that can be refused has been: group forces that were on stay on, as they were, after a refusal above)
  MdpGforce &h = c->gforce;
  MDP_TRY(mdp_postforce_commit(c, kStageGforce, kN * kLen, n, groupbit, h.cfg, cfg, sizeof *cfg));
  h.counted = true;
  return MDP_OK;
}

int mdp_gforce_run(mdp_ctx *c, long long first) { return c ? mdp_postforce_run(c, kStageGforce, first) : MDP_EINVAL; }

int mdp_gforce_state(mdp_ctx *c, int k, double *out)
{
  return c && out ? mdp_postforce_state(c, kStageGforce, k, kLen, out) : MDP_EINVAL;
}

int mdp_gforce_off(mdp_ctx *c) { return c ? mdp_postforce_off(c, kStageGforce) : MDP_EINVAL; }

} // extern "C"
