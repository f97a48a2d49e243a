// FIRE minimiser on the device: LAMMPS min_style fire (FIRE 2.0, Guenole et al., Comput. Mater. Sci. 175 (2020) 109584)
// with the eulerimplicit integrator, around the force computes of a resident context.  An iteration:
//   sums kernel     per-block partials of v.f, v.v, f.f in fixed slots, per-block maximum of |v_c|
//   control kernel  one workgroup: the fixed-order sums, the stop tests of the iteration before (its forces are the ones
//                   just summed), then the decisions of this iteration -- mix or zero, dt, alpha, dtv -- left in the
//                   control block (MdpFireWord) for the advance kernel; stop code, iteration and sum f.f also go to
//                   pinned host words
//   advance kernel  [x -= dtv_prev v / 2; v = 0]  v += dtv ftm2v f / m;  [v = s1 v + s2 f];  x += dtv v, with the
//                   displacement votes, the accumulator reset and the force clear of the integrate kernel (md.hip)
//   [reneighbouring when the vote of the iteration before asked for it]  ->  compute
// The sums are taken in a fixed order, so a minimisation is bitwise reproducible wherever the forces are.  The host
// never waits for a decision; once the stop code is latched, iterations that were queued too many change nothing.
#include "mdp_common.h"

#include <cmath>
#include <type_traits>

namespace {

struct FireArgs {
  int npart, peek, with_energy;
  double ftol, etol, maxiter, maxeval; // (the counts as doubles: the block counts in doubles)
  double dmax, dtmax, dtmin, delaystep, dtgrow, dtshrink, alpha0, alphashrink;
  int initialdelay;
  const double *acc; // acc[0]: the energy of the last compute (with_energy)
};

// MASK: held atoms (outside the integrate group, MdpGroupArgs) are left out of the sums and the maximum -- what LAMMPS
// sees with fix setforce 0 0 0 on them -- and still reach the shuffles and the block sum
template <bool MASK>
__global__ __launch_bounds__(256) void fire_sums_kernel(const int n, const double *__restrict__ v,
                                                        const double *__restrict__ f, double *__restrict__ part,
                                                        double *__restrict__ pmax, const MdpGroupArgs M)
{
  __shared__ double wmax[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double e[3] = {0.0, 0.0, 0.0}, m = 0.0;
  bool in = i < n;
  if constexpr (MASK)
    if (in) in = mdp_group_moves(M, mdp_group_mask(M, i));
  if (in) {
    const double vx = v[3 * (size_t) i], vy = v[3 * (size_t) i + 1], vz = v[3 * (size_t) i + 2];
    const double fx = f[3 * (size_t) i], fy = f[3 * (size_t) i + 1], fz = f[3 * (size_t) i + 2];
    e[0] = mdp_dot3(vx, fx, vy, fy, vz, fz);
    e[1] = mdp_dot3(vx, vx, vy, vy, vz, vz);
    e[2] = mdp_dot3(fx, fx, fy, fy, fz, fz);
    m = fmax(fabs(vx), fmax(fabs(vy), fabs(vz)));
  }
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64)); // (a maximum does not depend on the order)
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  mdp_block_sum_256<3>(e, part); // (every lane; its barrier also orders wmax)
  if (threadIdx.x == 0) pmax[blockIdx.x] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
}

// one workgroup.  peek: only sum f.f of the current forces goes to the block (a state read between iterations)
__global__ __launch_bounds__(256) void fire_control_kernel(const double *__restrict__ part, const double *__restrict__ pmax,
                                                           double *__restrict__ st, const FireArgs a,
                                                           double *__restrict__ pin)
{
  __shared__ double mx[256];
  double s[3];
  mdp_slot_sum_256<3>(part, a.npart, s);
  double m = 0.0;
  for (int b = threadIdx.x; b < a.npart; b += 256) m = fmax(m, pmax[b]);
  mx[threadIdx.x] = m;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int) threadIdx.x < h) mx[threadIdx.x] = fmax(mx[threadIdx.x], mx[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double vdotf = s[0], vv = s[1], ff = s[2];
  st[kFireFFnow] = ff;
  if (a.peek || st[kFireStop] != 0.0) return; // latched: the block stays as the stopping iteration left it
  double iter = st[kFireIter], dt = st[kFireDt], alpha = st[kFireAlpha], last_neg = st[kFireLastNeg];
  st[kFireFF] = ff;
  int stop = MDP_FIRE_RUNNING;
  if (iter > 0.0) { // the forces just summed are those of iteration `iter`: its stop tests
    const double neval = st[kFireNeval] + 1.0;
    st[kFireNeval] = neval;
    if (a.with_energy) {
      const double ep = st[kFireElast], e = a.acc[0];
      st[kFireEprev] = ep;
      st[kFireElast] = e;
      if (a.etol > 0.0 && iter - last_neg > a.delaystep && fabs(e - ep) < a.etol * 0.5 * (fabs(e) + fabs(ep) + 1.0e-8))
        stop = MDP_FIRE_ETOL;
    }
    if (!stop && sqrt(ff) < a.ftol) stop = MDP_FIRE_FTOL;
    if (!stop && neval >= a.maxeval) stop = MDP_FIRE_MAXEVAL;
  }
  if (!stop && iter >= a.maxiter) stop = MDP_FIRE_MAXITER;
  if (stop) {
    st[kFireStop] = (double) stop;
    pin[1] = iter;
    pin[2] = ff;
    pin[0] = (double) stop;
    return;
  }
  iter += 1.0;
  double s1 = 1.0, s2 = 0.0, vmax = mx[0];
  const bool mix = vdotf > 0.0;
  if (mix) {
    s1 = 1.0 - alpha;
    s2 = ff <= 1.0e-20 ? 0.0 : alpha * sqrt(vv / ff);
    if (iter - last_neg > a.delaystep) {
      dt = fmin(dt * a.dtgrow, a.dtmax);
      alpha *= a.alphashrink;
    }
  } else {
    last_neg = iter;
    st[kFireNneg] += 1.0;
    if (!(a.initialdelay && iter < a.delaystep)) {
      alpha = a.alpha0;
      if (dt * a.dtshrink >= a.dtmin) dt *= a.dtshrink;
    }
    vmax = 0.0; // (the velocities are zeroed before the step)
  }
  const double dtv = dt * vmax <= a.dmax ? dt : a.dmax / vmax;
  st[kFireDtvPrev] = st[kFireDtv];
  st[kFireDtv] = dtv;
  st[kFireS1] = s1;
  st[kFireS2] = s2;
  st[kFireMix] = mix ? 1.0 : 0.0;
  st[kFireZero] = mix ? 0.0 : 1.0;
  st[kFireDt] = dt;
  st[kFireAlpha] = alpha;
  st[kFireIter] = iter;
  st[kFireLastNeg] = last_neg;
  st[kFireVdotF] = vdotf;
  pin[1] = iter;
  pin[2] = ff;
}

// The step of one iteration, from the control block.  What it shares with nve_advance_kernel (md.hip): the accumulator
// reset of the compute that follows (SC.acc), the force clear of a style that accumulates (zero_f), CHECK and the style
// votes -- every lane reaches the votes.  The reach of an atom over the next two iterations is not dt |v| here: the step
// is chosen per iteration on the device, the velocities are mixed with the forces and start from rest after P <= 0.  One
// further iteration moves the atom by at most dtn (|v| + dtn |a| + s2 |f|) with dtn = min(dtgrow dt, dtmax), where the part
// from the velocity it has now is capped by dmax per component (the control kernel shortens dtv so that dtv max|v_c| <=
// dmax); the forces of this iteration stand for the next ones.  Two and a half of that, as in the integrate kernel.
// Once the stop code is latched the kernel moves nothing and votes for nothing; the resets still serve the compute.
// MASK: a held atom (outside the integrate group) keeps x and v; its force is cleared like any other, and it votes with
// the position it has and no reach.
template <bool CHECK, bool MASK>
__global__ __launch_bounds__(256) void fire_advance_kernel(const int nlocal, const double ftm2v, const double dmax,
                                                           const double dtgrow, const double dtmax, const int halfstepback,
                                                           const double *__restrict__ st, const double *__restrict__ rmass,
                                                           double *__restrict__ f, double *__restrict__ v,
                                                           double4 *__restrict__ xq, const mdp_hold_t *__restrict__ xhold,
                                                           const double trigsq, const double hardsq, int *__restrict__ flag,
                                                           const MdpStyleCheck SC, const int zero_f, const MdpGroupArgs M)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool t = false, h = false;
  MdpStyleVote w;
  if (SC.acc) { // what acc_zero_kernel does
    for (int k = i; k < SC.nacc; k += gridDim.x * 256) SC.acc[k] = 0.0;
    if (i == 0) {
      const int f0 = SC.flags[0];
      if (f0) SC.flags[4] |= f0;
      SC.flags[0] = 0;
      if (SC.ovf)
        for (int k = 0; k < MDP_NOVF_LISTS; k++) SC.ovf[(size_t) k * SC.ovf_stride] = 0;
    } else if (i < 4)
      SC.flags[i] = 0;
  }
  const bool live = st[kFireStop] == 0.0;
  if (i < nlocal) {
    const double fx = f[3 * (size_t) i], fy = f[3 * (size_t) i + 1], fz = f[3 * (size_t) i + 2];
    if (zero_f) {
      f[3 * (size_t) i] = 0.0;
      f[3 * (size_t) i + 1] = 0.0;
      f[3 * (size_t) i + 2] = 0.0;
    }
    bool held = false;
    if constexpr (MASK) held = !mdp_group_moves(M, mdp_group_mask(M, i));
    if (live && held) { // (MASK only)
      const double4 x = xq[i];
      if (CHECK) {
        const double dx = x.x - xhold[3 * (size_t) i], dy = x.y - xhold[3 * (size_t) i + 1], dz = x.z - xhold[3 * (size_t) i + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        t = d2 > trigsq;
        h = d2 > hardsq;
      }
      mdp_style_test(SC, (size_t) i, x, 0.0, w);
    } else if (live) {
      const double dtv = st[kFireDtv], s2 = st[kFireS2];
      double vx = v[3 * (size_t) i], vy = v[3 * (size_t) i + 1], vz = v[3 * (size_t) i + 2];
      double4 x = xq[i];
      if (st[kFireZero] != 0.0) { // P <= 0: half a step back along the old velocity, then rest
        if (halfstepback) {
          const double hb = 0.5 * st[kFireDtvPrev];
          x.x -= hb * vx;
          x.y -= hb * vy;
          x.z -= hb * vz;
        }
        vx = vy = vz = 0.0;
      }
      const double s = dtv * ftm2v / rmass[i];
      vx += s * fx;
      vy += s * fy;
      vz += s * fz;
      if (st[kFireMix] != 0.0) {
        const double s1 = st[kFireS1];
        vx = s1 * vx + s2 * fx;
        vy = s1 * vy + s2 * fy;
        vz = s1 * vz + s2 * fz;
      }
      v[3 * (size_t) i] = vx;
      v[3 * (size_t) i + 1] = vy;
      v[3 * (size_t) i + 2] = vz;
      x.x += dtv * vx;
      x.y += dtv * vy;
      x.z += dtv * vz;
      xq[i] = x;
      double two_steps = 0.0;
      if (CHECK || SC.xa || SC.xp) {
        const double dtn = fmin(st[kFireDt] * dtgrow, dtmax);
        const double vn = sqrt(vx * vx + vy * vy + vz * vz), fn = sqrt(fx * fx + fy * fy + fz * fz);
        const double one = fmin(dtn * vn, 1.7320508075688772 * dmax) + dtn * (dtn * ftm2v / rmass[i] + s2) * fn;
        two_steps = 2.5 * one;
      }
      if (CHECK) {
        const double dx = x.x - xhold[3 * (size_t) i], dy = x.y - xhold[3 * (size_t) i + 1], dz = x.z - xhold[3 * (size_t) i + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        t = d2 > trigsq || mdp_reaches(d2, hardsq, two_steps);
        h = d2 > hardsq;
      }
      mdp_style_test(SC, (size_t) i, x, two_steps, w);
    }
  }
  if (CHECK) { // (pinned host words zeroed by the host before the launch: plain idempotent stores)
    const bool wt = __any(t), wh = __any(h);
    if ((threadIdx.x & 63) == 0) {
      if (wt) flag[0] = 1;
      if (wh) flag[1] = 1;
    }
  }
  mdp_style_vote(SC, w, 0);
}

// mdp_fire_setup with an integrate group: the moving atoms start from rest, the held ones keep their velocities
__global__ void fire_rest_kernel(const int n, double *__restrict__ v, const MdpGroupArgs M)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 3 * n) return;
  if (mdp_group_moves(M, mdp_group_mask(M, k / 3))) v[k] = 0.0;
}

double *fire_pin(mdp_ctx *c) { return c->h_pinned + kPinFire; }

// the sums of the current v and f, then the control kernel (peek: sum f.f alone)
int fire_sums_control(mdp_ctx *c, bool peek)
{
  MdpFire &F = c->fire;
  const mdp_fire_config &g = F.cfg;
  hipStream_t st = c->stream;
  const int n = c->nlocal, nb = n ? nblk(n) : 0;
  bool masked = false;
  MdpGroupArgs M;
  MDP_TRY(mdp_group_args(c, &masked, &M));
  MDP_HIP(c, F.part.reserve((size_t) 4 * nb + 4));
  if (n && masked) fire_sums_kernel<true><<<nb, 256, 0, st>>>(n, c->v.p, c->f.p, F.part.p, F.part.p + 3 * (size_t) nb, M);
  else if (n) fire_sums_kernel<false><<<nb, 256, 0, st>>>(n, c->v.p, c->f.p, F.part.p, F.part.p + 3 * (size_t) nb, M);
  FireArgs a;
  a.npart = nb;
  a.peek = peek ? 1 : 0;
  a.with_energy = g.etol > 0.0 ? 1 : 0;
  a.ftol = g.ftol;
  a.etol = g.etol;
  a.maxiter = (double) g.maxiter;
  a.maxeval = (double) g.maxeval;
  a.dmax = g.dmax;
  a.dtmax = g.tmax * F.dt0;
  a.dtmin = g.tmin * F.dt0;
  a.delaystep = (double) g.delaystep;
  a.dtgrow = g.dtgrow;
  a.dtshrink = g.dtshrink;
  a.alpha0 = g.alpha0;
  a.alphashrink = g.alphashrink;
  a.initialdelay = g.initialdelay;
  a.acc = c->acc.p;
  fire_control_kernel<<<1, 256, 0, st>>>(F.part.p, F.part.p + 3 * (size_t) nb, F.st.p, a, fire_pin(c));
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

// the energy of the current positions by a compute of its own; the forces stay as they were (an energy compute may round
// them differently, and the next iteration must see the forces of its own compute)
int fire_energy_now(mdp_ctx *c, double *e)
{
  MdpFire &F = c->fire;
  const size_t nf = (size_t) 3 * c->nall;
  MDP_HIP(c, F.fsave.reserve(nf + 3));
  if (nf) MDP_HIP(c, hipMemcpyAsync(F.fsave.p, c->f.p, sizeof(double) * nf, hipMemcpyDeviceToDevice, c->stream));
  MDP_TRY(mdp_md_compute(c, 1, 0));
  if (nf) MDP_HIP(c, hipMemcpyAsync(c->f.p, F.fsave.p, sizeof(double) * nf, hipMemcpyDeviceToDevice, c->stream));
  double th[9];
  MDP_TRY(mdp_md_thermo(c, th)); // (waits for the stream, checks the overflow flags)
  *e = th[1];
  return MDP_OK;
}

} // namespace

int mdp_fire_launch_advance(mdp_ctx *c, int *flag, double trigsq, double hardsq, const MdpStyleCheck &sc, bool zero_f)
{
  const int n = c->nlocal;
  if (!n) return MDP_OK;
  const MdpFire &F = c->fire;
  const mdp_fire_config &g = F.cfg;
  const double dtmax = g.tmax * F.dt0;
  bool masked = false;
  MdpGroupArgs M;
  MDP_TRY(mdp_group_args(c, &masked, &M));
  auto launch = [&](auto cv, auto mv) {
    fire_advance_kernel<decltype(cv)::value, decltype(mv)::value><<<nblk(n), 256, 0, c->stream>>>(
        n, c->cfg.ftm2v, g.dmax, g.dtgrow, dtmax, g.halfstepback, F.st.p, c->rmass.p, c->f.p, c->v.p, c->xq.p, c->xhold.p,
        flag ? trigsq : 0.0, flag ? hardsq : 0.0, flag, sc, zero_f ? 1 : 0, M);
  };
  constexpr std::true_type T;
  constexpr std::false_type F_;
  if (flag) {
    if (masked) launch(T, T);
    else launch(T, F_);
  } else {
    if (masked) launch(F_, T);
    else launch(F_, F_);
  }
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

extern "C" {

int mdp_fire_setup(mdp_ctx *c, const mdp_fire_config *cfg)
{
  if (!c || !cfg) return MDP_EINVAL;
  if (!c->md) return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup: mdp_md_setup not called (the minimiser needs a resident context)");
  if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup: mdp_dd_setup not called (the minimiser reneighbours through the one-brick calls)");
  if (c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup: the minimiser runs on one rank only (this context is a brick of %d ranks)",
                    c->dd.G.nranks);
  if (c->nhc.on || c->lgv.on)
    return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup: a thermostat (%s) is on; switch it off first",
                    c->nhc.on ? "mdp_nhc_setup" : "mdp_langevin_setup");
  if (c->heat.on) return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup: heat sources (mdp_heat_setup) are on; mdp_heat_off first");
  MDP_TRY(mdp_refuse_if_on(c, "mdp_fire_setup", kRefuseOffFirst));
  if (!c->neigh_set) return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup: neighbor list not built (mdp_dd_reneighbor)");
  if (!(cfg->etol >= 0.0) || !(cfg->ftol >= 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: etol and ftol must be >= 0");
  if (cfg->maxiter < 0 || cfg->maxeval < 0) return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: maxiter and maxeval must be >= 0");
  if (!(cfg->dmax > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: dmax must be > 0");
  if (!(cfg->tmax >= 1.0) || !(cfg->tmin > 0.0) || !(cfg->tmin <= 1.0))
    return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: tmax must be >= 1 and tmin in (0, 1]");
  if (cfg->delaystep < 0) return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: delaystep must be >= 0");
  if (!(cfg->dtgrow >= 1.0) || !(cfg->dtshrink > 0.0) || !(cfg->dtshrink <= 1.0))
    return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: dtgrow must be >= 1 and dtshrink in (0, 1]");
  if (!(cfg->alpha0 > 0.0) || !(cfg->alpha0 < 1.0) || !(cfg->alphashrink > 0.0) || !(cfg->alphashrink <= 1.0))
    return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: alpha0 must be in (0, 1) and alphashrink in (0, 1]");
  if (!(c->cfg.dt > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_fire_setup: the context's time step must be > 0");
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(mdp_md_flush_final(c)); // (a final half the host deferred belongs to the run before)
  MdpFire &F = c->fire;
  F.on = false;
  F.cfg = *cfg;
  F.dt0 = c->cfg.dt;
  MDP_HIP(c, F.st.reserve(kFireWords));
  bool masked = false;
  MdpGroupArgs M;
  MDP_TRY(mdp_group_args(c, &masked, &M));
  if (c->nlocal && masked) {
    fire_rest_kernel<<<nblk(3 * (long long) c->nlocal), 256, 0, c->stream>>>(c->nlocal, c->v.p, M);
    MDP_HIP(c, hipGetLastError());
  } else if (c->nlocal)
    MDP_HIP(c, hipMemsetAsync(c->v.p, 0, sizeof(double) * 3 * (size_t) c->nlocal, c->stream));
  MDP_TRY(mdp_md_compute(c, 1, 0));
  double th[9];
  MDP_TRY(mdp_md_thermo(c, th));
  F.e_initial = th[1];
  double blk[kFireWords] = {};
  blk[kFireDtv] = blk[kFireDtvPrev] = blk[kFireDt] = F.dt0;
  blk[kFireS1] = 1.0;
  blk[kFireAlpha] = cfg->alpha0;
  blk[kFireEprev] = blk[kFireElast] = F.e_initial;
  MDP_TRY(mdp_write_small(c, F.st.p, blk, sizeof blk));
  MDP_TRY(fire_sums_control(c, true));
  double ff = 0.0;
  MDP_TRY(mdp_read_one(c, F.st.p + kFireFFnow, sizeof ff, &ff));
  F.fnorm_initial = sqrt(ff);
  F.e_cache = F.e_initial;
  F.e_cache_iter = 0;
  F.reneighbors0 = c->dd.reneighbors;
  F.late = 0;
  double *pin = fire_pin(c);
  pin[0] = pin[1] = 0.0;
  pin[2] = ff;
  F.on = true;
  return MDP_OK;
}

int mdp_fire_iterate(mdp_ctx *c, long long n, int *stop)
{
  if (!c) return MDP_EINVAL;
  if (!c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup not called");
  MDP_HIP(c, hipSetDevice(c->device));
  const volatile double *pin = fire_pin(c);
  const int eflag = c->fire.cfg.etol > 0.0 ? 1 : 0;
  for (long long k = 0; k < n; k++) {
    // (no wait: the word is what the last control kernel the host has waited behind -- through the displacement check's
    // event, an iteration late -- left there)
    if (pin[0] != 0.0) break;
    MDP_TRY(fire_sums_control(c, false));
    int moved = 0, dangerous = 0;
    MDP_TRY(mdp_md_integrate_check(c, 0, &moved, &dangerous));
    if (dangerous) c->fire.late++;
    if (moved) MDP_TRY(mdp_dd_reneighbor(c));
    MDP_TRY(mdp_md_compute(c, eflag, 0));
  }
  if (stop) *stop = (int) pin[0];
  return MDP_OK;
}

int mdp_fire_state(mdp_ctx *c, double *out)
{
  if (!c || !out) return MDP_EINVAL;
  if (!c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_fire_setup not called");
  MDP_HIP(c, hipSetDevice(c->device));
  MdpFire &F = c->fire;
  double blk[kFireWords];
  MDP_TRY(mdp_read_one(c, F.st.p, sizeof blk, blk)); // (waits for the stream)
  if (blk[kFireStop] == 0.0) { // the control kernel of the next iteration has not summed the current forces yet
    MDP_TRY(fire_sums_control(c, true));
    MDP_TRY(mdp_read_one(c, F.st.p + kFireFFnow, sizeof(double), &blk[kFireFFnow]));
  } else
    blk[kFireFFnow] = blk[kFireFF];
  double e_prev = blk[kFireEprev], e_last = blk[kFireElast];
  if (!(F.cfg.etol > 0.0)) {
    if (F.e_cache_iter != (long long) blk[kFireIter]) {
      MDP_TRY(fire_energy_now(c, &F.e_cache));
      F.e_cache_iter = (long long) blk[kFireIter];
    }
    e_prev = e_last = F.e_cache;
  }
  out[0] = blk[kFireStop];
  out[1] = blk[kFireIter];
  out[2] = blk[kFireNeval];
  out[3] = blk[kFireDt];
  out[4] = blk[kFireAlpha];
  out[5] = sqrt(blk[kFireFFnow]);
  out[6] = F.e_initial;
  out[7] = e_prev;
  out[8] = e_last;
  out[9] = (double) (c->dd.reneighbors - F.reneighbors0);
  out[10] = blk[kFireDtv];
  out[11] = blk[kFireDtvPrev];
  out[12] = blk[kFireS1];
  out[13] = blk[kFireS2];
  out[14] = blk[kFireMix];
  out[15] = blk[kFireZero];
  out[16] = blk[kFireLastNeg];
  out[17] = blk[kFireNneg];
  out[18] = blk[kFireVdotF];
  out[19] = F.fnorm_initial;
  out[20] = (double) F.late;
  return MDP_OK;
}

int mdp_fire_off(mdp_ctx *c)
{
  if (!c) return MDP_EINVAL;
  c->fire.on = false; // (the context's dt was never touched; v stays as the minimiser left it)
  return MDP_OK;
}

} // extern "C"
