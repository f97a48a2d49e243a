// Nose-Hoover chain thermostat on the device: LAMMPS fix nvt (FixNH, Martyna-Tuckerman-Klein chain, thermostat only)
// around the velocity-Verlet kernels of md.hip.  A step with the thermostat:
//   initial half:  [chain kernel: H with the temperature carried from the last half-update]  ->  integrate kernel
//                  (v = S v + dtf f/m; x += dt v), S read from device memory
//   final half:    kick + partial sums of m v^2  ->  chain kernel (T from the partials, H)  ->  v *= S
//   fused final(n) + initial(n+1):  partial sums of (v + dtf f/m), not stored  ->  chain kernel (H of step n, H of
//                  step n+1, S = S_final S_initial)  ->  integrate kernel with both kicks and S in between
// The partial sums sit in fixed per-block slots and the chain kernel adds them in a fixed order: the temperature, and so
// the trajectory, is bitwise reproducible (no float atomics).  The host never waits for the temperature.
#include "mdp_common.h"

#include <cmath>

namespace {

// w_i = v_i (+ dtf / m_i f_i if KICK; stored if STORE); part[block] = sum over the block of m_i |w_i|^2 in a fixed order
// MASK: over the integrate group alone (MdpGroupArgs) -- the other atoms are left as they are and add 0 to the sum,
// which every lane still reaches
template <bool KICK, bool STORE, bool MASK>
__global__ __launch_bounds__(256) void nhc_ke_kernel(const int n, const double dtf, const double *__restrict__ rmass,
                                                     const double *__restrict__ f, double *__restrict__ v,
                                                     double *__restrict__ part, const MdpGroupArgs M)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  double e = 0.0;
  bool in = i < n;
  if constexpr (MASK)
    if (in) in = mdp_group_moves(M, mdp_group_mask(M, i));
  if (in) {
    double vx = v[3 * (size_t) i], vy = v[3 * (size_t) i + 1], vz = v[3 * (size_t) i + 2];
    if (KICK) { // the same expressions as the integrate kernels' final half-kick
      const double s = dtf / rmass[i];
      vx += s * f[3 * (size_t) i];
      vy += s * f[3 * (size_t) i + 1];
      vz += s * f[3 * (size_t) i + 2];
    }
    if (STORE) {
      v[3 * (size_t) i] = vx;
      v[3 * (size_t) i + 1] = vy;
      v[3 * (size_t) i + 2] = vz;
    }
    e = rmass[i] * (vx * vx + vy * vy + vz * vz);
  }
  mdp_block_sum_256(e, part);
}

__global__ void nhc_scale_kernel(const int n, const double *__restrict__ st, double *__restrict__ v)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * n) return;
  v[i] *= st[kNhcS];
}

// the same for the atoms of the integrate group alone
__global__ void nhc_scale_group_kernel(const int n, const double *__restrict__ st, double *__restrict__ v, const MdpGroupArgs M)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 3 * n) return;
  if (mdp_group_moves(M, mdp_group_mask(M, k / 3))) v[k] *= st[kNhcS];
}

// the launch of nhc_ke_kernel with or without the group
template <bool KICK, bool STORE>
void nhc_ke_launch(mdp_ctx *c, const int n, const double dtf, const bool masked, const MdpGroupArgs &M)
{
  MdpNhc &h = c->nhc;
  if (masked)
    nhc_ke_kernel<KICK, STORE, true><<<nblk(n), 256, 0, c->stream>>>(n, dtf, c->rmass.p, c->f.p, c->v.p, h.part.p, M);
  else
    nhc_ke_kernel<KICK, STORE, false><<<nblk(n), 256, 0, c->stream>>>(n, dtf, c->rmass.p, c->f.p, c->v.p, h.part.p, M);
}

enum { kNhcSetup = 1, kNhcFinal = 2, kNhcInitial = 4 };

struct NhcArgs {
  int mode, npart, M, L;
  double dt, tfreq, tdrag, nf, kb, mvv2e;
  double tt_a; // target of the setup / final half-update
  double tt_b; // target of the initial half-update
};

// state layout: [0] T  [1] Tt  [2] energy  [3..11) eta  [11..20) eta_dot  [20..28) eta_dotdot  [28..36) Q  [36] S
__device__ void nhc_masses(double *st, const NhcArgs &a, double tt)
{
  double *Q = st + kNhcQ;
  const double kt = a.kb * tt, tf2 = a.tfreq * a.tfreq;
  Q[0] = a.nf * kt / tf2;
  for (int i = 1; i < a.M; i++) Q[i] = kt / tf2;
}

__device__ void nhc_energy(double *st, const NhcArgs &a, double tt)
{
  const double *eta = st + 3, *ed = st + 11, *Q = st + kNhcQ;
  const double kt = a.kb * tt;
  double e = a.nf * kt * eta[0] + 0.5 * Q[0] * ed[0] * ed[0];
  for (int i = 1; i < a.M; i++) e += kt * eta[i] + 0.5 * Q[i] * ed[i] * ed[i];
  st[1] = tt;
  st[2] = e;
}

// one half-update of the chain (FixNH::nhc_temp_integrate) at target tt; T is updated in place; returns the factor
__device__ double nhc_half(double *st, const NhcArgs &a, double tt, double &T)
{
  double *eta = st + 3, *ed = st + 11, *edd = st + 20, *Q = st + kNhcQ;
  const int M = a.M;
  const double kt = a.kb * tt, ket = a.nf * kt;
  nhc_masses(st, a, tt);
  edd[0] = Q[0] > 0.0 ? (a.nf * a.kb * T - ket) / Q[0] : 0.0;
  const double w = 1.0 / a.L;
  const double dt2 = w * a.dt / 2.0, dt4 = w * a.dt / 4.0, dt8 = w * a.dt / 8.0;
  double S = 1.0;
  for (int l = 0; l < a.L; l++) {
    double e;
    for (int i = M - 1; i > 0; i--) {
      e = exp(-dt8 * ed[i + 1]);
      ed[i] = ((ed[i] * e + edd[i] * dt4) * a.tdrag) * e;
    }
    e = exp(-dt8 * ed[1]);
    ed[0] = ((ed[0] * e + edd[0] * dt4) * a.tdrag) * e;
    const double s = exp(-dt2 * ed[0]);
    S *= s;
    T *= s * s;
    edd[0] = Q[0] > 0.0 ? (a.nf * a.kb * T - ket) / Q[0] : 0.0;
    for (int i = 0; i < M; i++) eta[i] += dt2 * ed[i];
    ed[0] = (ed[0] * e + edd[0] * dt4) * e;
    for (int i = 1; i < M; i++) {
      e = exp(-dt8 * ed[i + 1]);
      ed[i] *= e;
      edd[i] = (Q[i - 1] * ed[i - 1] * ed[i - 1] - kt) / Q[i];
      ed[i] += edd[i] * dt4;
      ed[i] *= e;
    }
  }
  return S;
}

// one workgroup: the fixed-order sum of the partials (setup / final), then the chain on one lane
__global__ __launch_bounds__(256) void nhc_chain_kernel(const double *__restrict__ part, double *__restrict__ st,
                                                        const NhcArgs a)
{
  double T = 0.0;
  if (a.mode & (kNhcSetup | kNhcFinal)) { // (the mode is the same for every lane: all of them reach the sum)
    double mv2;
    mdp_slot_sum_256<1>(part, a.npart, &mv2);
    const double ke = 0.5 * a.mvv2e * mv2;
    T = a.nf > 0.0 ? 2.0 * ke / (a.nf * a.kb) : 0.0;
  }
  if (threadIdx.x != 0) return;
  if (!(a.mode & (kNhcSetup | kNhcFinal))) T = st[0]; // carried over from the last half-update (already scaled)
  double S = 1.0;
  if (a.mode & kNhcSetup) { // FixNH::setup
    double *ed = st + 11, *edd = st + 20, *Q = st + kNhcQ;
    nhc_masses(st, a, a.tt_a);
    for (int i = 1; i < a.M; i++) edd[i] = (Q[i - 1] * ed[i - 1] * ed[i - 1] - a.kb * a.tt_a) / Q[i];
    nhc_energy(st, a, a.tt_a);
  }
  if (a.mode & kNhcFinal) {
    S *= nhc_half(st, a, a.tt_a, T);
    nhc_energy(st, a, a.tt_a);
  }
  if (a.mode & kNhcInitial) {
    S *= nhc_half(st, a, a.tt_b, T);
    nhc_energy(st, a, a.tt_b);
  }
  st[0] = T;
  st[kNhcS] = S;
}

double nhc_target(const MdpNhc &h, long long n)
{
  const double delta = h.last == h.first ? 0.0 : (double) (n - h.first) / (double) (h.last - h.first);
  return h.cfg.t_start + delta * (h.cfg.t_stop - h.cfg.t_start);
}

NhcArgs nhc_args(const mdp_ctx *c, int mode, int npart, double tt_a, double tt_b)
{
  const mdp_nhc_config &g = c->nhc.cfg;
  const double dt = mdp_step(c).dt;
  NhcArgs a;
  a.mode = mode;
  a.npart = npart;
  a.M = g.tchain;
  a.L = g.tloop;
  a.dt = dt;
  a.tfreq = 1.0 / g.t_period;
  a.tdrag = 1.0 - dt * a.tfreq * g.drag / g.tloop;
  a.nf = g.nf;
  a.kb = g.boltz;
  a.mvv2e = g.mvv2e;
  a.tt_a = tt_a;
  a.tt_b = tt_b;
  return a;
}

int nhc_reserve(mdp_ctx *c, int n)
{
  MDP_HIP(c, c->nhc.part.reserve((size_t) nblk(n) + 1));
  return MDP_OK;
}

} // namespace

int mdp_nhc_open(mdp_ctx *c, bool with_final, const double **vscale)
{
  MdpNhc &h = c->nhc;
  hipStream_t st = c->stream;
  const int n = c->nlocal;
  const double dtf = mdp_step(c).dtf;
  bool masked = false;
  MdpGroupArgs M;
  MDP_TRY(mdp_group_args(c, &masked, &M));
  MDP_TRY(nhc_reserve(c, n));
  int mode = kNhcInitial;
  double tt_a = h.tt;
  if (with_final) {
    mode |= kNhcFinal; // H of the finished step at its own target
    if (n) nhc_ke_launch<true, false>(c, n, dtf, masked, M);
  } else if (h.need_setup) {
    mode |= kNhcSetup;
    tt_a = nhc_target(h, h.step);
    if (n) nhc_ke_launch<false, false>(c, n, dtf, masked, M);
    h.need_setup = false;
  }
  h.step++;
  h.tt = nhc_target(h, h.step);
  nhc_chain_kernel<<<1, 256, 0, st>>>(h.part.p, h.st.p, nhc_args(c, mode, n ? nblk(n) : 0, tt_a, h.tt));
  MDP_HIP(c, hipGetLastError());
  *vscale = h.st.p + kNhcS;
  return MDP_OK;
}

int mdp_nhc_final(mdp_ctx *c)
{
  MdpNhc &h = c->nhc;
  hipStream_t st = c->stream;
  const int n = c->nlocal;
  bool masked = false;
  MdpGroupArgs M;
  MDP_TRY(mdp_group_args(c, &masked, &M));
  MDP_TRY(nhc_reserve(c, n));
  if (n) nhc_ke_launch<true, true>(c, n, mdp_step(c).dtf, masked, M);
  nhc_chain_kernel<<<1, 256, 0, st>>>(h.part.p, h.st.p, nhc_args(c, kNhcFinal, n ? nblk(n) : 0, h.tt, h.tt));
  if (n && masked) nhc_scale_group_kernel<<<nblk(3 * (long long) n), 256, 0, st>>>(n, h.st.p, c->v.p, M);
  else if (n) nhc_scale_kernel<<<nblk(3 * (long long) n), 256, 0, st>>>(n, h.st.p, c->v.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

extern "C" {

int mdp_nhc_setup(mdp_ctx *c, const mdp_nhc_config *cfg)
{
  if (!c || !cfg) return MDP_EINVAL;
  if (c->lgv.on)
    return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup: the Langevin thermostat (mdp_langevin_setup) is on; one thermostat per context");
  if (c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup: a minimisation (mdp_fire_setup) is on; mdp_fire_off first");
  if (c->heat.on) return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup: heat sources (mdp_heat_setup) are on; mdp_heat_off first");
  MDP_TRY(mdp_refuse_if_on(c, "mdp_nhc_setup", kRefuseOffFirst));
  if (c->dd.on && c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup: the thermostat runs on one rank only (this context is a brick of %d ranks)",
                    c->dd.G.nranks);
  if (!(cfg->t_start > 0.0) || !(cfg->t_stop > 0.0))
    return mdp_fail(c, MDP_EINVAL, "mdp_nhc_setup: Tstart and Tstop must be > 0");
  if (!(cfg->t_period > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_nhc_setup: Tdamp must be > 0");
  if (cfg->tchain < 1 || cfg->tchain > MDP_NHC_MAXCHAIN)
    return mdp_fail(c, MDP_EINVAL, "mdp_nhc_setup: tchain must be in 1..%d", MDP_NHC_MAXCHAIN);
  if (cfg->tloop < 1) return mdp_fail(c, MDP_EINVAL, "mdp_nhc_setup: tloop must be >= 1");
  if (!(cfg->drag >= 0.0) || !(cfg->nf >= 0.0) || !(cfg->boltz > 0.0) || !(cfg->mvv2e > 0.0))
    return mdp_fail(c, MDP_EINVAL, "mdp_nhc_setup: drag, nf, boltz or mvv2e out of range");
  MDP_HIP(c, hipSetDevice(c->device));
  MdpNhc &h = c->nhc;
  MDP_HIP(c, h.st.reserve(kNhcWords));
  double zero[kNhcWords] = {};
  zero[kNhcS] = 1.0;
  MDP_TRY(mdp_write_small(c, h.st.p, zero, sizeof zero)); // the chain starts at rest
  h.cfg = *cfg;
  h.first = h.last = h.step = 0;
  h.tt = cfg->t_start;
  h.need_setup = true;
  h.on = true;
  return MDP_OK;
}

int mdp_nhc_run(mdp_ctx *c, long long first, long long last)
{
  if (!c) return MDP_EINVAL;
  if (!c->nhc.on) return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup not called");
  if (last < first) return mdp_fail(c, MDP_EINVAL, "mdp_nhc_run: last step %lld before first %lld", last, first);
  // a final half the host deferred belongs to the step before the new ramp: it runs now, at that step's target
  MDP_TRY(mdp_md_flush_final(c));
  MdpNhc &h = c->nhc;
  h.first = first;
  h.last = last;
  h.step = first;
  h.tt = nhc_target(h, first);
  h.need_setup = true;
  return MDP_OK;
}

int mdp_nhc_state(mdp_ctx *c, double *out)
{
  if (!c || !out) return MDP_EINVAL;
  if (!c->nhc.on) return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup not called");
  MDP_HIP(c, hipSetDevice(c->device));
  return mdp_read_one(c, c->nhc.st.p, sizeof(double) * MDP_NHC_STATE_LEN, out);
}

int mdp_nhc_set_state(mdp_ctx *c, const double *in)
{
  if (!c || !in) return MDP_EINVAL;
  if (!c->nhc.on) return mdp_fail(c, MDP_ESTATE, "mdp_nhc_setup not called");
  MDP_HIP(c, hipSetDevice(c->device));
  double s[MDP_NHC_STATE_LEN];
  MDP_TRY(mdp_read_one(c, c->nhc.st.p, sizeof s, s));
  const int M = c->nhc.cfg.tchain;
  for (int i = 0; i < MDP_NHC_MAXCHAIN; i++) { // (links beyond the chain stay at rest: eta_dot[M] == 0)
    s[3 + i] = i < M ? in[3 + i] : 0.0;
    s[11 + i] = i < M ? in[11 + i] : 0.0;
    s[20 + i] = i < M ? in[20 + i] : 0.0;
  }
  s[19] = 0.0;
  return mdp_write_small(c, c->nhc.st.p, s, sizeof s);
}

int mdp_nhc_off(mdp_ctx *c)
{
  if (!c) return MDP_EINVAL;
  // a deferred final half of the last thermostatted step completes with its chain update before the NVE code takes over
  if (c->nhc.on) MDP_TRY(mdp_md_flush_final(c));
  c->nhc.on = false;
  return MDP_OK;
}

} // extern "C"
