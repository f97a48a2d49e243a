// Tether springs on the device: LAMMPS fix spring tether (FixSpring::spring_tether) with a tether point that moves at a
// constant velocity (the constant-velocity mode of fix smd), in front of every kick that first consumes a compute's
// forces.  For the forces of step n the tether point is p = c + vel (n - first) dt, and with xu = x + h . image
// (mdp_unwrap) over the atoms of the spring's group
//   M = sum m,  xcm = (sum m xu) / M,  d = xcm - p (0 in a dimension that takes no part),  r = max(|d|, 1e-10),
//   dr = r - R0,  F = K d dr / r,  E = K dr^2 / 2,  f_i -= (F / M) m_i,  ftotal = (-Fx, -Fy, -Fz, sign(dr) |F|)
// in three launches: per block and spring sum m xu, sum m (in two exact parts) and the atom count in fixed slots
// (spring_sums_kernel); one workgroup that adds the slots in a fixed order and leaves the state words and F / M of every
// spring in device memory (spring_control_kernel); one lane per owned atom that takes (F / M) m off its f, spring after
// spring (spring_apply_kernel).  No float atomics and no host wait: a run is bitwise reproducible.  The springs are the
// second post-force stage of a context, behind the indenters (kMdpStages, mdp_common.h): mdp_postforce_apply calls
// mdp_spring_pass, and postforce.hip holds the life cycle they share with the indenters.
#include "mdp_common.h"

#include <cmath>

namespace {

constexpr int kN = MDP_SPRING_MAX;
constexpr int kLen = MDP_SPRING_STATE_LEN;

// the group bits of the springs that are on, under the name the kernels take them by
struct SpringBits : MdpSlotBits {};

// part[kSprW b + 5 k + j]: the sums over block b of m xu, m yu, m zu, m_hi and m_lo of spring k's atoms; cnt[kN b + k]: their
// number.  m = m_hi + m_lo with m_hi the multiple of 2^-20 nearest m: for up to 2^22 atoms with masses in [1, 2048) both
// sums are exact in any order (53 bits each), so M = sum m_hi + sum m_lo is the correctly rounded sum of the masses
// whatever order the device holds the atoms in; outside that range it is a sum like the others.  A block takes
// kSprPer x 256 consecutive atoms, a lane kSprPer of them at a stride of 256 (coalesced), added in that order (fma: one
// rounding per term, the same in every build).  Every lane reaches the block sum; a block with no atom of any spring
// writes zeros.  The counts are integers: a wave adds its ballots' bit counts in LDS
constexpr int kSprPer = 4;
__global__ __launch_bounds__(256) void spring_sums_kernel(const int n, const double4 *__restrict__ xq, const int *__restrict__ image,
                                                          const double *__restrict__ rmass, const int *__restrict__ mask,
                                                          const SpringBits B, const DdGeom G, double *__restrict__ part,
                                                          int *__restrict__ cnt)
{
  __shared__ int wcnt[kN];
  if (threadIdx.x < kN) wcnt[threadIdx.x] = 0;
  __syncthreads();
  double e[kSprW];
#pragma unroll
  for (int q = 0; q < kSprW; q++) e[q] = 0.0;
  int seen = 0;
#pragma unroll
  for (int j = 0; j < kSprPer; j++) {
    const int i = (blockIdx.x * kSprPer + j) * 256 + threadIdx.x;
    int in = 0;
    if (i < n) {
      const int w = B.any ? mask[i] : 0;
#pragma unroll
      for (int k = 0; k < kN; k++)
        if (k < B.n && (!B.bit[k] || (w & B.bit[k]))) in |= 1 << k;
    }
#pragma unroll
    for (int k = 0; k < kN; k++) { // (every lane votes: the ballot is the wave's)
      const int c = __popcll(__ballot((in >> k) & 1));
      if (c && (threadIdx.x & 63) == 0) atomicAdd(&wcnt[k], c);
    }
    if (!in) continue;
    seen |= in;
    double xu[3];
    mdp_unwrap(G, xq[i], image[i], xu);
    const double m = rmass[i];
    const double mhi = rint(m * 0x1p20) * 0x1p-20, mlo = m - mhi;
#pragma unroll
    for (int k = 0; k < kN; k++) {
      const bool mine = (in >> k) & 1;
      const double mk = mine ? m : 0.0;
      e[5 * k] = fma(mk, xu[0], e[5 * k]);
      e[5 * k + 1] = fma(mk, xu[1], e[5 * k + 1]);
      e[5 * k + 2] = fma(mk, xu[2], e[5 * k + 2]);
      e[5 * k + 3] += mine ? mhi : 0.0;
      e[5 * k + 4] += mine ? mlo : 0.0;
    }
  }
  mdp_block_sum_256_seen<kN>(e, seen, part);
  if (threadIdx.x < kN) cnt[kN * (size_t) blockIdx.x + threadIdx.x] = wcnt[threadIdx.x]; // (behind the block sum's barrier)
}

struct SpringCtl {
  int n = 0;
  double step = 0.0;
  double k[kN], r0[kN], p[kN][3]; // p: the tether point of this step
  int use[kN][3];
};

// one workgroup: the fixed-order sums, then lane 0 forms xcm, F, E and ftotal of every spring that is on and leaves
// F / M of the pass at st[kSprF + 4 k ..]
__global__ __launch_bounds__(256) void spring_control_kernel(const double *__restrict__ part, const int *__restrict__ cnt,
                                                             const int npart, const SpringCtl a, double *__restrict__ st)
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
  double s[kSprW];
  mdp_slot_sum_256<kSprW>(part, npart, s); // (its barriers stand between the atomics above and lane 0's reads below)
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < kN; k++) {
    if (k >= a.n) continue;
    const double M = s[5 * k + 3] + s[5 * k + 4];
    const bool has = M > 0.0; // (a group that lost its atoms to a new mask: no centre of mass, no force)
    const double xc = has ? s[5 * k] / M : 0.0, yc = has ? s[5 * k + 1] / M : 0.0, zc = has ? s[5 * k + 2] / M : 0.0;
    const double dx = a.use[k][0] ? xc - a.p[k][0] : 0.0, dy = a.use[k][1] ? yc - a.p[k][1] : 0.0,
                 dz = a.use[k][2] ? zc - a.p[k][2] : 0.0;
    double r = sqrt(mdp_dot3(dx, dx, dy, dy, dz, dz));
    r = r > 1.0e-10 ? r : 1.0e-10;
    const double dr = r - a.r0[k];
    const double fx = has ? a.k[k] * dx * dr / r : 0.0, fy = has ? a.k[k] * dy * dr / r : 0.0, fz = has ? a.k[k] * dz * dr / r : 0.0;
    const double fm = sqrt(mdp_dot3(fx, fx, fy, fy, fz, fz));
    double *w = st + k * kLen;
    w[0] = has ? 0.5 * a.k[k] * dr * dr : 0.0;
    w[1] = 0.0 - fx;
    w[2] = 0.0 - fy;
    w[3] = 0.0 - fz;
    w[4] = dr < 0.0 ? 0.0 - fm : fm;
    w[5] = a.step;
    w[6] = xc;
    w[7] = yc;
    w[8] = zc;
    w[9] = a.p[k][0];
    w[10] = a.p[k][1];
    w[11] = a.p[k][2];
    w[12] = M;
    w[13] = (double) atoms[k];
    w[14] += 1.0;
    w[15] = 0.0;
    double *g = st + kSprF + 4 * k;
    g[0] = has ? fx / M : 0.0;
    g[1] = has ? fy / M : 0.0;
    g[2] = has ? fz / M : 0.0;
  }
}

// f_i -= (F / M) m_i, spring after spring in the order of their slots (fma: one rounding per spring, the same in every
// build); an atom in no spring is neither read nor written
__global__ __launch_bounds__(256) void spring_apply_kernel(const int n, double *__restrict__ f, const double *__restrict__ rmass,
                                                           const int *__restrict__ mask, const SpringBits B,
                                                           const double *__restrict__ st)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int w = B.any ? mask[i] : 0;
  int in = 0;
#pragma unroll
  for (int k = 0; k < kN; k++)
    if (k < B.n && (!B.bit[k] || (w & B.bit[k]))) in |= 1 << k;
  if (!in) return;
  const double m = rmass[i];
  double fx = f[3 * (size_t) i], fy = f[3 * (size_t) i + 1], fz = f[3 * (size_t) i + 2];
#pragma unroll
  for (int k = 0; k < kN; k++) {
    if (!((in >> k) & 1)) continue;
    const double *g = st + kSprF + 4 * k;
    fx = fma(-g[0], m, fx);
    fy = fma(-g[1], m, fy);
    fz = fma(-g[2], m, fz);
  }
  f[3 * (size_t) i] = fx;
  f[3 * (size_t) i + 1] = fy;
  f[3 * (size_t) i + 2] = fz;
}

// the counts of a set-up: [k] atoms of spring k, [kN + k] those of them with a mass > 0
__global__ void spring_count_kernel(const int n, const int *__restrict__ mask, const double *__restrict__ rmass, const SpringBits B,
                                    int *__restrict__ count)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int w = B.any ? mask[i] : 0;
#pragma unroll
  for (int k = 0; k < kN; k++)
    if (k < B.n && (!B.bit[k] || (w & B.bit[k]))) {
      atomicAdd(count + k, 1);
      if (rmass[i] > 0.0) atomicAdd(count + kN + k, 1);
    }
}

} // namespace

int mdp_spring_pass(mdp_ctx *c)
{
  MdpSpring &h = c->spring;
  const SpringBits B = mdp_slot_bits<SpringBits>(h.n, h.bit);
  if (B.any && !mdp_mask_current(c))
    return mdp_fail(c, MDP_ESTATE, "integrate: a spring acts on a group but no mask covers the current atoms (mdp_md_set_mask)");
  if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "springs are on (mdp_spring_setup) but the context has no box any more");
  if (!c->image_set) return mdp_fail(c, MDP_ESTATE, "springs are on (mdp_spring_setup) but the image flags were withdrawn (mdp_md_set_image)");
  const int n = c->nlocal, nb = nblk(n), nbs = nblk(n, 256 * kSprPer);
  MDP_HIP(c, h.part.reserve((size_t) kSprW * (nbs ? nbs : 1)));
  MDP_HIP(c, h.cpart.reserve((size_t) kN * (nbs ? nbs : 1)));
  const double t = (double) h.nhalf * mdp_step(c).dt;
  SpringCtl a;
  a.n = h.n;
  a.step = (double) (h.first + h.nhalf);
  for (int k = 0; k < kN; k++) {
    const mdp_spring_config &q = h.cfg[k < h.n ? k : 0];
    a.k[k] = q.k;
    a.r0[k] = q.r0;
    for (int d = 0; d < 3; d++) {
      a.use[k][d] = q.use[d] ? 1 : 0;
      a.p[k][d] = q.use[d] ? q.c[d] + q.vel[d] * t : 0.0;
    }
  }
  if (n) spring_sums_kernel<<<nbs, 256, 0, c->stream>>>(n, c->xq.p, c->image.p, c->rmass.p, c->mask.p, B, c->dd.G, h.part.p,
                                                            h.cpart.p);
  spring_control_kernel<<<1, 256, 0, c->stream>>>(h.part.p, h.cpart.p, nbs, a, h.st.p);
  if (n) spring_apply_kernel<<<nb, 256, 0, c->stream>>>(n, c->f.p, c->rmass.p, c->mask.p, B, h.st.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

extern "C" {

int mdp_spring_setup(mdp_ctx *c, int n, const mdp_spring_config *cfg, const int *groupbit)
{
  if (!c || !cfg || !groupbit) return MDP_EINVAL;
  if (n < 1 || n > kN) return mdp_fail(c, MDP_EINVAL, "mdp_spring_setup: %d springs; a context takes 1 to %d", n, kN);
  for (int k = 0; k < n; k++) {
    const mdp_spring_config &q = cfg[k];
    if (!std::isfinite(q.k) || q.k < 0.0) return mdp_fail(c, MDP_EINVAL, "mdp_spring_setup: spring %d: K must be finite and >= 0", k);
    if (!std::isfinite(q.r0) || q.r0 < 0.0) return mdp_fail(c, MDP_EINVAL, "mdp_spring_setup: spring %d: R0 must be finite and >= 0", k);
    for (int d = 0; d < 3; d++)
      if (!std::isfinite(q.c[d]) || !std::isfinite(q.vel[d]))
        return mdp_fail(c, MDP_EINVAL, "mdp_spring_setup: spring %d: tether point and velocity must be finite", k);
    if (!q.use[0] && !q.use[1] && !q.use[2])
      return mdp_fail(c, MDP_EINVAL, "mdp_spring_setup: spring %d: no dimension takes part (use is all zero)", k);
  }
  MDP_TRY(mdp_postforce_refuse_setup(c, kStageSpring));
  if (!c->md)
    return mdp_fail(c, MDP_ESTATE, "mdp_spring_setup: springs need a resident context (mdp_md_setup): on a host-linked one the host keeps the image flags");
  if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "mdp_spring_setup: mdp_dd_setup not called (the unwrapped positions need the box of the brick)");
  if (!c->image_set) return mdp_fail(c, MDP_ESTATE, "mdp_spring_setup: no image set (mdp_md_set_image)");
  const SpringBits B = mdp_slot_bits<SpringBits>(n, groupbit);
  if (B.any && !mdp_mask_current(c))
    return mdp_fail(c, MDP_ESTATE, "mdp_spring_setup: a spring acts on a group but no mask covers the current atoms (mdp_md_set_mask)");
  MDP_HIP(c, hipSetDevice(c->device));
  MdpSpring &h = c->spring;
  { // every spring's group holds an atom and a mass (reads only: springs that are on stay as they are after a refusal)
    MDP_HIP(c, h.count.reserve(2 * kN));
    const int zero[2 * kN] = {};
    MDP_TRY(mdp_write_small(c, h.count.p, zero, sizeof zero));
    const int na = c->nlocal;
    if (na) spring_count_kernel<<<nblk(na), 256, 0, c->stream>>>(na, c->mask.p, c->rmass.p, B, h.count.p);
    MDP_HIP(c, hipGetLastError());
    int cnt[2 * kN];
    MDP_TRY(mdp_read_one(c, h.count.p, sizeof cnt, cnt));
    for (int k = 0; k < n; k++) {
      if (!cnt[k]) return mdp_fail(c, MDP_ESTATE, "mdp_spring_setup: spring %d has no atoms (group bit %d): it has no centre of mass", k, groupbit[k]);
      if (!cnt[kN + k])
        return mdp_fail(c, MDP_ESTATE, "mdp_spring_setup: the %d atoms of spring %d (group bit %d) have no mass", cnt[k], k, groupbit[k]);
    }
  }
  // (everything that can be refused has been: springs that were on stay on, as they were, after a refusal above)
  return mdp_postforce_commit(c, kStageSpring, kSprTotal, n, groupbit, h.cfg, cfg, sizeof *cfg);
}

int mdp_spring_run(mdp_ctx *c, long long first) { return c ? mdp_postforce_run(c, kStageSpring, first) : MDP_EINVAL; }

int mdp_spring_state(mdp_ctx *c, int k, double *out)
{
  return c && out ? mdp_postforce_state(c, kStageSpring, k, kLen, out) : MDP_EINVAL;
}

int mdp_spring_off(mdp_ctx *c) { return c ? mdp_postforce_off(c, kStageSpring) : MDP_EINVAL; }

} // extern "C"
