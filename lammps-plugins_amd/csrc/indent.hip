// Indenters on the device: LAMMPS fix indent (FixIndent::post_force with `units box`) for spheres, cylinders and planes
// whose centre moves at a constant velocity, in front of every kick that first consumes a compute's forces.  For the
// forces of step n the centre is ctr = c + vel (n - first) dt, and with D = x - ctr through Domain::minimum_image
//   sphere, cylinder (D's component along the axis zeroed before the minimum image, as LAMMPS does):
//            r = |D|,  dr = r - R (side out) or R - r (side in),  dr < 0:  f += -+ K dr^2 D / r
//   plane:   dr = x[dim] - c[dim] (lo) or c[dim] - x[dim] (hi),   dr < 0:  f[dim] += +- K dr^2
//   energy -= K/3 dr^3,  force on the indenter -= the atom's force;  r == 0: no force, the energy is counted
// in two launches: one lane per owned atom that adds the forces of every indenter into f and leaves, per block and
// indenter, energy, force and contact count in fixed slots (indent_force_kernel); one workgroup that adds the slots in a
// fixed order and leaves the state of every indenter in device memory (indent_control_kernel).  No float atomics and no
// host wait: a run is bitwise reproducible.  The indenters are the first post-force stage of a context (kMdpStages,
// mdp_common.h): mdp_postforce_apply calls mdp_indent_pass, and postforce.hip holds the life cycle they share with the springs.
#include "mdp_common.h"

#include <cmath>

namespace {

constexpr int kI = MDP_INDENT_MAX;
constexpr int kLen = MDP_INDENT_STATE_LEN;

// everything the force kernel needs, by value: uniform over the grid, so it stays in scalar registers
struct IndentArgs {
  int n = 0;                        // indenters on
  int shape[kI], dim[kI], side[kI], bit[kI];
  double k[kI], r[kI], c[kI][3];    // c: the centre of this step
  double h[6] = {1, 1, 1, 0, 0, 0}; // xprd, yprd, zprd, yz, xz, xy (Domain::h)
  int per[3] = {1, 1, 1};
};

__device__ __forceinline__ double pick3(const int d, const double a, const double b, const double c) { return d == 0 ? a : d == 1 ? b : c; }

// Domain::minimum_image (triclinic; an orthogonal box has no tilt and the three wraps are independent)
__device__ __forceinline__ void indent_minimum_image(const IndentArgs &A, double &dx, double &dy, double &dz)
{
  if (A.per[2] && fabs(dz) > 0.5 * A.h[2]) {
    const double s = dz < 0.0 ? 1.0 : -1.0;
    dz += s * A.h[2];
    dy += s * A.h[3];
    dx += s * A.h[4];
  }
  if (A.per[1] && fabs(dy) > 0.5 * A.h[1]) {
    const double s = dy < 0.0 ? 1.0 : -1.0;
    dy += s * A.h[1];
    dx += s * A.h[5];
  }
  if (A.per[0] && fabs(dx) > 0.5 * A.h[0]) dx += dx < 0.0 ? A.h[0] : -A.h[0];
}

// part[kIndW b + 5 k + j]: over block b, indenter k's energy, the sum of the forces it put on atoms (x, y, z) and the number
// of atoms it touches.  One lane per owned atom; a lane loops over the indenters that are on and only a lane in contact
// with one reads and writes its f.  Every lane reaches the block sum; a block without contact writes zeros
__global__ __launch_bounds__(256) void indent_force_kernel(const int n, const double4 *__restrict__ xq, double *__restrict__ f,
                                                           const IndentArgs A, double *__restrict__ part, const MdpGroupArgs M)
{
  double e[kIndW];
#pragma unroll
  for (int q = 0; q < kIndW; q++) e[q] = 0.0;
  int seen = 0;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double4 x = xq[i];
    const int m = M.mask ? mdp_group_mask(M, i) : 0;
    double fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll
    for (int k = 0; k < kI; k++) {
      if (k >= A.n || (A.bit[k] && !(m & A.bit[k]))) continue;
      const int dim = A.dim[k];
      double dr, gx = 0.0, gy = 0.0, gz = 0.0;
      if (A.shape[k] == MDP_INDENT_PLANE) {
        const double d = pick3(dim, x.x, x.y, x.z) - A.c[k][dim];
        dr = A.side[k] ? -d : d;
        const double fm = A.side[k] ? -(A.k[k] * dr * dr) : A.k[k] * dr * dr;
        gx = dim == 0 ? fm : 0.0;
        gy = dim == 1 ? fm : 0.0;
        gz = dim == 2 ? fm : 0.0;
      } else {
        const bool cyl = A.shape[k] == MDP_INDENT_CYLINDER;
        double dx = cyl && dim == 0 ? 0.0 : x.x - A.c[k][0];
        double dy = cyl && dim == 1 ? 0.0 : x.y - A.c[k][1];
        double dz = cyl && dim == 2 ? 0.0 : x.z - A.c[k][2];
        indent_minimum_image(A, dx, dy, dz);
        const double r = sqrt(mdp_dot3(dx, dx, dy, dy, dz, dz));
        dr = A.side[k] ? A.r[k] - r : r - A.r[k];
        const double fm = A.side[k] ? -(A.k[k] * dr * dr) : A.k[k] * dr * dr;
        const double s = r > 0.0 ? fm / r : 0.0;
        gx = dx * s;
        gy = dy * s;
        gz = dz * s;
      }
      if (dr < 0.0) {
        seen |= 1 << k;
        e[5 * k] = -(A.k[k] / 3.0) * dr * dr * dr;
        e[5 * k + 1] = gx;
        e[5 * k + 2] = gy;
        e[5 * k + 3] = gz;
        e[5 * k + 4] = 1.0;
        fx += gx;
        fy += gy;
        fz += gz;
      }
    }
    if (seen) {
      f[3 * (size_t) i] += fx;
      f[3 * (size_t) i + 1] += fy;
      f[3 * (size_t) i + 2] += fz;
    }
  }
  mdp_block_sum_256_seen<kI>(e, seen, part);
}

struct IndentCtl {
  int n = 0;
  double step = 0.0;
  double c[kI][3];
};

// one workgroup: the fixed-order sums, then lane 0 leaves the state words of every indenter that is on
__global__ __launch_bounds__(256) void indent_control_kernel(const double *__restrict__ part, const int npart, const IndentCtl a,
                                                             double *__restrict__ st)
{
  double s[kIndW];
  mdp_slot_sum_256<kIndW>(part, npart, s);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < kI; k++) {
    if (k >= a.n) continue;
    double *w = st + k * kLen;
    w[0] = s[5 * k];
    w[1] = 0.0 - s[5 * k + 1]; // the force on the indenter: minus what it put on the atoms
    w[2] = 0.0 - s[5 * k + 2];
    w[3] = 0.0 - s[5 * k + 3];
    w[4] = s[5 * k + 4];
    w[5] = a.step;
    w[6] = a.c[k][0];
    w[7] = a.c[k][1];
    w[8] = a.c[k][2];
    w[9] += 1.0;
  }
}

// the context's own box and periodicity: a brick's (resident, or host-linked with bricks), else the box a host-linked
// context was handed (one periodic rank)
bool indent_box(const mdp_ctx *c, double h[6], int per[3])
{
  if (c->dd.on) {
    for (int k = 0; k < 6; k++) h[k] = c->dd.G.h[k];
    for (int d = 0; d < 3; d++) per[d] = c->dd.G.nonper[d] ? 0 : 1;
    return true;
  }
  if (!c->md && c->host_box_set) {
    for (int k = 0; k < 6; k++) h[k] = c->host_h[k];
    per[0] = per[1] = per[2] = 1;
    return true;
  }
  return false;
}

int indent_no_mask(mdp_ctx *c, const char *who)
{
  return mdp_fail(c, MDP_ESTATE, "%s: an indenter acts on a group but no mask covers the current atoms (%s)", who,
                  c->md ? "mdp_md_set_mask" : "mdp_hnve_set_mask after mdp_set_atoms_host");
}

} // namespace

int mdp_indent_pass(mdp_ctx *c)
{
  MdpIndent &h = c->indent;
  IndentArgs A;
  const int any = mdp_slot_bits(h.n, h.bit).any;
  if (any && !mdp_mask_current(c)) return indent_no_mask(c, "integrate");
  if (!indent_box(c, A.h, A.per)) return mdp_fail(c, MDP_ESTATE, "indenters are on (mdp_indent_setup) but the context has no box any more");
  const int n = c->nlocal, nb = nblk(n);
  MDP_HIP(c, h.part.reserve((size_t) kIndW * (nb ? nb : 1)));
  const double t = (double) h.nhalf * mdp_step(c).dt;
  IndentCtl a;
  A.n = a.n = h.n;
  a.step = (double) (h.first + h.nhalf);
  for (int k = 0; k < kI; k++) {
    const mdp_indent_config &q = h.cfg[k < h.n ? k : 0];
    A.shape[k] = q.shape;
    A.dim[k] = q.dim;
    A.side[k] = q.side;
    A.bit[k] = k < h.n ? h.bit[k] : 0;
    A.k[k] = q.k;
    A.r[k] = q.r;
    for (int d = 0; d < 3; d++) A.c[k][d] = a.c[k][d] = q.c[d] + q.vel[d] * t;
  }
  const MdpGroupArgs M = any ? mdp_mask_args(c) : MdpGroupArgs();
  if (n) indent_force_kernel<<<nb, 256, 0, c->stream>>>(n, c->xq.p, c->f.p, A, h.part.p, M);
  indent_control_kernel<<<1, 256, 0, c->stream>>>(h.part.p, nb, a, h.st.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

extern "C" {

int mdp_indent_setup(mdp_ctx *c, int n, const mdp_indent_config *cfg, const int *groupbit)
{
  if (!c || !cfg || !groupbit) return MDP_EINVAL;
  if (n < 1 || n > kI) return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: %d indenters; a context takes 1 to %d", n, kI);
  for (int k = 0; k < n; k++) {
    const mdp_indent_config &q = cfg[k];
    if (q.shape < MDP_INDENT_SPHERE || q.shape > MDP_INDENT_PLANE)
      return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: shape %d is none of sphere (0), cylinder (1), plane (2)", k, q.shape);
    if (q.dim < 0 || q.dim > 2) return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: dim %d is not 0, 1 or 2", k, q.dim);
    if (q.side < 0 || q.side > 1) return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: side %d is not 0 (out, lo) or 1 (in, hi)", k, q.side);
    if (!std::isfinite(q.k) || q.k < 0.0) return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: K must be finite and >= 0", k);
    if (!std::isfinite(q.r) || q.r < 0.0) return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: R must be finite and >= 0", k);
    for (int d = 0; d < 3; d++)
      if (!std::isfinite(q.c[d]) || !std::isfinite(q.vel[d]))
        return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: centre and velocity must be finite", k);
    if (q.shape == MDP_INDENT_CYLINDER && q.vel[q.dim] != 0.0)
      return mdp_fail(c, MDP_EINVAL, "mdp_indent_setup: indenter %d: a cylinder cannot move along its axis (vel[%d] = %g)", k, q.dim, q.vel[q.dim]);
  }
  MDP_TRY(mdp_postforce_refuse_setup(c, kStageIndent));
  if (!c->md && !c->hn_on) return mdp_fail(c, MDP_ESTATE, "mdp_indent_setup: no integrator on the context (mdp_md_setup or mdp_hnve_setup)");
  double hbox[6];
  int per[3];
  if (!indent_box(c, hbox, per))
    return mdp_fail(c, MDP_ESTATE, "mdp_indent_setup: no box on the context (%s)", c->md ? "mdp_dd_setup" : "mdp_set_box_host");
  if (mdp_slot_bits(n, groupbit).any && !mdp_mask_current(c)) return indent_no_mask(c, "mdp_indent_setup");
  // (everything that can be refused has been: indenters that were on stay on, as they were, after a refusal above)
  MDP_HIP(c, hipSetDevice(c->device));
  return mdp_postforce_commit(c, kStageIndent, kI * kLen, n, groupbit, c->indent.cfg, cfg, sizeof *cfg);
}

int mdp_indent_run(mdp_ctx *c, long long first) { return c ? mdp_postforce_run(c, kStageIndent, first) : MDP_EINVAL; }

int mdp_indent_state(mdp_ctx *c, int k, double *out)
{
  return c && out ? mdp_postforce_state(c, kStageIndent, k, kLen, out) : MDP_EINVAL;
}

int mdp_indent_off(mdp_ctx *c) { return c ? mdp_postforce_off(c, kStageIndent) : MDP_EINVAL; }

} // extern "C"
