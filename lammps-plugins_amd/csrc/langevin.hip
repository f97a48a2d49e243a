// Langevin thermostat on the device: LAMMPS fix langevin (FixLangevin::post_force without gjf / angmom / omega, zero
// and tally included) inside the velocity-Verlet kernels of md.hip.  The Langevin force of step n,
//   f_L = gfactor1[t] v + gfactor2[t] sqrt(T(n)) (u - 0.5)   (u per component, v after the initial half of step n),
// is added in registers by the kernel that first reads the forces of the step's compute:
//   fused final(n) + initial(n+1):  both half-kicks with f + f_L (nve_advance_kernel, LANGEVIN)
//   first initial half of a run:    the setup force (Fix::setup) at the run's first step, phase 1 of the noise
//   a final half on its own:        f + f_L written back (lgv_final_kernel), for the initial half that follows
// The noise is Philox4x32-10 keyed by (seed, atom tag, step, phase): no state per atom or per rank, so the trajectory
// is the same in any atom order and on any number of ranks.  zero yes: a pre-pass sums the random parts in fixed
// per-block slots and one workgroup divides their fixed-order sum by natoms; tally yes: the integrate kernel leaves
// per-block sums of f_L . v and one workgroup adds them to the energy, on the device.  No float atomics and no host
// wait: a run is bitwise reproducible.
#include "mdp_common.h"

#include <cmath>

namespace {

// zero yes: part[3 b + k] = the sum over block b of the random parts fran_k of the step (mdp_lgv_random)
// MASK: of the Langevin group's atoms alone (MdpGroupArgs); the others add 0 and still reach the block sum
template <bool MASK>
__global__ __launch_bounds__(256) void lgv_zero_kernel(const int n, const MdpLgvArgs L, double *__restrict__ part,
                                                       const MdpGroupArgs M)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  double r[3] = {0.0, 0.0, 0.0};
  bool in = i < n;
  if constexpr (MASK)
    if (in) in = mdp_group_lgv(M, mdp_group_mask(M, i));
  if (in) mdp_lgv_random(L, i, r[0], r[1], r[2]);
  mdp_block_sum_256<3>(r, part);
}

// zero yes: st[kLgvMean + k] = (sum of the random parts) / natoms; the three components in one pass over the slots
__global__ __launch_bounds__(256) void lgv_mean_kernel(const double *__restrict__ part, const int npart,
                                                       const double natoms, double *__restrict__ st)
{
  double s[3];
  mdp_slot_sum_256<3>(part, npart, s);
  if (threadIdx.x < 3) st[kLgvMean + threadIdx.x] = (threadIdx.x == 0 ? s[0] : (threadIdx.x == 1 ? s[1] : s[2])) / natoms;
}

// tally yes: E = the fixed-order sum of the partials of f_L . v; the setup force starts the energy of the run at
// 0.5 E dt (FixLangevin::compute_scalar at beginstep), a step adds E dt (end_of_step)
__global__ __launch_bounds__(256) void lgv_tally_kernel(const double *__restrict__ part, const int npart, const double dt,
                                                        const int setup, double *__restrict__ st)
{
  double e;
  mdp_slot_sum_256<1>(part, npart, &e);
  if (threadIdx.x == 0) {
    st[kLgvE] = setup ? 0.5 * e * dt : st[kLgvE] + e * dt;
    st[kLgvElast] = e;
  }
}

double lgv_target(const MdpLangevin &h, long long n)
{
  double delta = h.last == h.first ? 0.0 : (double) (n - h.first) / (double) (h.last - h.first);
  delta = delta < 0.0 ? 0.0 : (delta > 1.0 ? 1.0 : delta); // (steps beyond `last` hold Tstop: T never goes negative)
  return h.cfg.t_start + delta * (h.cfg.t_stop - h.cfg.t_start);
}

// the per-type factors of FixLangevin::init for this time step and unit system (rewritten when they change)
int lgv_tables(mdp_ctx *c)
{
  MdpLangevin &h = c->lgv;
  const MdpStep s = mdp_step(c);
  const double dt = s.dt, ftm2v = s.ftm2v, *mass = s.mass;
  if (h.tab_dt == dt && h.tab_ftm2v == ftm2v) return MDP_OK;
  const mdp_langevin_config &g = h.cfg;
  double tab[2 * 16] = {};
  for (int t = 1; t < 16; t++) {
    const double m = mass[t] > 0.0 ? mass[t] : 0.0;
    tab[t] = -m / g.t_period / ftm2v;
    tab[kLgvG2 + t] = sqrt(m) * sqrt(24.0 * g.boltz / g.t_period / dt / g.mvv2e) / ftm2v;
    tab[t] *= 1.0 / g.ratio[t];
    tab[kLgvG2 + t] *= 1.0 / sqrt(g.ratio[t]);
  }
  MDP_TRY(mdp_write_small(c, h.st.p, tab, sizeof tab));
  h.tab_dt = dt;
  h.tab_ftm2v = ftm2v;
  return MDP_OK;
}

} // namespace

int mdp_lgv_open(mdp_ctx *c, bool with_final, bool initial, bool *apply, MdpLgvArgs *L)
{
  MdpLangevin &h = c->lgv;
  const int n = c->nlocal;
  const bool setup = initial && !with_final && h.need_setup;
  *apply = !initial || with_final || setup;
  if (*apply) {
    MDP_TRY(lgv_tables(c));
    const int nb = nblk(n);
    MDP_HIP(c, h.part.reserve((size_t) 4 * nb + 4));
    L->tag = c->tag.p;
    L->type = c->type.p;
    L->perm = !c->md && c->host_sort ? c->host_perm.p : nullptr; // host mode: tags and types are in the host's order
    L->st = h.st.p;
    L->tsqrt = sqrt(lgv_target(h, h.step));
    L->seed = (unsigned) h.cfg.seed;
    L->lo = (unsigned) (unsigned long long) h.step;
    L->hi = (unsigned) ((unsigned long long) h.step >> 32);
    L->phase = setup ? 1u : 0u;
    L->mean = nullptr;
    L->part = h.cfg.tally ? h.part.p + (size_t) 3 * nb : nullptr;
    if (h.cfg.zero) {
      bool masked = false;
      MdpGroupArgs M;
      MDP_TRY(mdp_group_args(c, &masked, &M));
      if (n && masked) lgv_zero_kernel<true><<<nb, 256, 0, c->stream>>>(n, *L, h.part.p, M);
      else if (n) lgv_zero_kernel<false><<<nb, 256, 0, c->stream>>>(n, *L, h.part.p, M);
      lgv_mean_kernel<<<1, 256, 0, c->stream>>>(h.part.p, n ? nb : 0, (double) h.cfg.natoms, h.st.p);
      MDP_HIP(c, hipGetLastError());
      L->mean = h.st.p + kLgvMean;
    }
  }
  if (initial) {
    h.need_setup = false;
    h.step++;
  }
  return MDP_OK;
}

int mdp_lgv_close(mdp_ctx *c, const MdpLgvArgs &L)
{
  if (!L.part) return MDP_OK;
  lgv_tally_kernel<<<1, 256, 0, c->stream>>>(L.part, c->nlocal ? nblk(c->nlocal) : 0, mdp_step(c).dt, L.phase == 1u ? 1 : 0,
                                             c->lgv.st.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

extern "C" {

int mdp_langevin_setup(mdp_ctx *c, const mdp_langevin_config *cfg)
{
  if (!c || !cfg) return MDP_EINVAL;
  if (c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup: a minimisation (mdp_fire_setup) is on; mdp_fire_off first");
  if (c->nhc.on)
    return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup: the Nose-Hoover chain (mdp_nhc_setup) is on; one thermostat per context");
  if ((cfg->zero || cfg->tally) && c->dd.on && c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup: zero and tally run on one rank only (this context is a brick of %d ranks)",
                    c->dd.G.nranks);
  if (cfg->seed <= 0) return mdp_fail(c, MDP_EINVAL, "mdp_langevin_setup: the seed must be > 0");
  if (!(cfg->t_period > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_langevin_setup: damp must be > 0");
  if (!(cfg->t_start >= 0.0) || !(cfg->t_stop >= 0.0))
    return mdp_fail(c, MDP_EINVAL, "mdp_langevin_setup: Tstart and Tstop must be >= 0");
  for (int t = 1; t < 16; t++)
    if (!(cfg->ratio[t] > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_langevin_setup: the scale ratio of type %d must be > 0", t);
  if (!(cfg->boltz > 0.0) || !(cfg->mvv2e > 0.0) || (cfg->zero && cfg->natoms < 1))
    return mdp_fail(c, MDP_EINVAL, "mdp_langevin_setup: boltz, mvv2e or natoms out of range");
  MDP_HIP(c, hipSetDevice(c->device));
  MdpLangevin &h = c->lgv;
  MDP_HIP(c, h.st.reserve(kLgvWords));
  double zero[kLgvWords] = {};
  MDP_TRY(mdp_write_small(c, h.st.p, zero, sizeof zero));
  h.cfg = *cfg;
  h.tab_dt = h.tab_ftm2v = 0.0; // (the factors are computed by the first kernel that needs them)
  h.first = h.last = h.step = 0;
  h.need_setup = true;
  h.on = true;
  return MDP_OK;
}

int mdp_langevin_run(mdp_ctx *c, long long first, long long last)
{
  if (!c) return MDP_EINVAL;
  if (!c->lgv.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup not called");
  if (last < first) return mdp_fail(c, MDP_EINVAL, "mdp_langevin_run: last step %lld before first %lld", last, first);
  // a final half the host deferred belongs to the step before the new run: it runs now, with that step's force
  MDP_TRY(mdp_md_flush_final(c));
  MdpLangevin &h = c->lgv;
  h.first = first;
  h.last = last;
  h.step = first;
  h.need_setup = true;
  return MDP_OK;
}

int mdp_langevin_tally(mdp_ctx *c, double *out)
{
  if (!c || !out) return MDP_EINVAL;
  if (!c->lgv.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup not called");
  if (!c->lgv.cfg.tally) {
    *out = 0.0;
    return MDP_OK;
  }
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(mdp_md_flush_final(c)); // (the energy of the finished step)
  double e[2];
  MDP_TRY(mdp_read_one(c, c->lgv.st.p + kLgvE, sizeof e, e));
  *out = -(e[0] - 0.5 * e[1] * mdp_step(c).dt); // FixLangevin::compute_scalar: back from mid-step to the last full step
  return MDP_OK;
}

int mdp_langevin_off(mdp_ctx *c)
{
  if (!c) return MDP_EINVAL;
  // a deferred final half of the last thermostatted step completes with its Langevin force before NVE takes over
  if (c->lgv.on) MDP_TRY(mdp_md_flush_final(c));
  c->lgv.on = false;
  return MDP_OK;
}

} // extern "C"
