// Constant-flux heat sources on the device: LAMMPS fix heat (FixHeat::end_of_step with a constant eflux and no region)
// behind every final half that completes a step of the velocity-Verlet kernels of md.hip.  Source k adds
//   heat = eflux_k nevery_k dt ftm2v
// to the kinetic energy its group has about its centre of mass, every nevery_k steps:
//   ke = (0.5 sum m v.v mvv2e) ftm2v,  vcm = sum m v / M,  t = 0.5 vcm.vcm M,  escale = ((ke - t) + heat) / (ke - t),
//   scale = sqrt(escale),  v = scale v - (scale - 1) vcm                               (sums over the atoms of the group)
// in three launches: the sums of every source in one pass over the owned atoms, per block in fixed slots
// (heat_sums_kernel); one workgroup that adds the slots in a fixed order and leaves scale and vsub = (scale - 1) vcm of
// every source in device memory (heat_control_kernel); the pass that rescales (heat_apply_kernel).  A lane picks its
// source from the mask word by compare/select, as the Langevin baths do: lanes of different sources run the same code.
// No float atomics and no host wait: a run is bitwise reproducible.  escale < 0 or a denominator that is not positive
// latches (step, source) in the error words; from then on every source keeps scale 1 and vsub 0, and the next call that
// waits for the stream anyway reports it (mdp_heat_check).
#include "mdp_common.h"

#include <cmath>

namespace {

constexpr int kS = MDP_HEAT_MAXSRC;

// the group bits of the sources; a slot beyond nsrc has bit 0 and is never picked
struct HeatBits {
  int bit[kS] = {0, 0, 0, 0};
  int any = 0;
};

// the source of an atom with mask m (the groups are disjoint: at most one bit matches); only meaningful if m & B.any
__device__ __forceinline__ int heat_src(const HeatBits &B, int m)
{
  int k = 0;
  k = (m & B.bit[1]) ? 1 : k;
  k = (m & B.bit[2]) ? 2 : k;
  k = (m & B.bit[3]) ? 3 : k;
  return k;
}

// part[kHeatW b + 5 k + j]: the sums over block b of m v.v, m vx, m vy, m vz and m of source k's atoms.  A block takes
// kHeatPer x 256 consecutive atoms, a lane kHeatPer of them at a stride of 256 (coalesced), added in that order: a quarter
// of the slots for the control workgroup to read and a quarter of the shuffles.  Every lane reaches the block sum; an
// atom in no source adds 0 to all sums
constexpr int kHeatPer = 4;
__global__ __launch_bounds__(256) void heat_sums_kernel(const int n, const double *__restrict__ rmass, const double *__restrict__ v,
                                                        const HeatBits B, double *__restrict__ part, const MdpGroupArgs M)
{
  double e[kHeatW];
#pragma unroll
  for (int q = 0; q < kHeatW; q++) e[q] = 0.0;
  int seen = 0;
#pragma unroll
  for (int j = 0; j < kHeatPer; j++) {
    const int i = (blockIdx.x * kHeatPer + j) * 256 + threadIdx.x;
    int k = 0;
    double m = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
    if (i < n) {
      const int w = mdp_group_mask(M, i);
      if (w & B.any) {
        k = heat_src(B, w);
        seen |= 1 << k;
        m = rmass[i];
        vx = v[3 * (size_t) i];
        vy = v[3 * (size_t) i + 1];
        vz = v[3 * (size_t) i + 2];
      }
    }
    const double mvv = m * mdp_dot3(vx, vx, vy, vy, vz, vz), mx = m * vx, my = m * vy, mz = m * vz;
#pragma unroll
    for (int b = 0; b < kS; b++) {
      e[5 * b] += k == b ? mvv : 0.0;
      e[5 * b + 1] += k == b ? mx : 0.0;
      e[5 * b + 2] += k == b ? my : 0.0;
      e[5 * b + 3] += k == b ? mz : 0.0;
      e[5 * b + 4] += k == b ? m : 0.0;
    }
  }
  mdp_block_sum_256_seen<kS>(e, seen, part);
}

// what the one workgroup needs besides the partials
struct HeatCtl {
  double heat[kS] = {0.0, 0.0, 0.0, 0.0};   // eflux nevery dt ftm2v
  double kefac[kS] = {0.0, 0.0, 0.0, 0.0};  // ke = (kefac sum m v.v) ftm2v, kefac = 0.5 mvv2e
  double ftm2v = 0.0, step = 0.0;
  int due = 0;                              // bit k: source k is applied at this step
  int nsrc = 0, mass = 0;                   // mass: M of every source is taken from this pass's sums
};

// one workgroup: the fixed-order sums, then lane 0 forms vcm, escale, scale and vsub of every source that is due.  A bad
// escale in ANY source of the step latches before anything is stored, so the outcome does not hang on the sources' order
__global__ __launch_bounds__(256) void heat_control_kernel(const double *__restrict__ part, const int npart, const HeatCtl a,
                                                           double *__restrict__ st)
{
  double s[kHeatW];
  mdp_slot_sum_256<kHeatW>(part, npart, s);
  if (threadIdx.x != 0) return;
  double scale[kS], vcm[kS][3], den[kS], mass[kS];
  bool latched = st[kHeatErr] != 0.0;
  int bad = -1;
#pragma unroll
  for (int k = 0; k < kS; k++) {
    scale[k] = 1.0;
    den[k] = 0.0;
    vcm[k][0] = vcm[k][1] = vcm[k][2] = 0.0;
    mass[k] = a.mass ? s[5 * k + 4] : st[k * kHeatWords + kHeatM];
    if (k < a.nsrc && ((a.due >> k) & 1)) {
      const double ke = (a.kefac[k] * s[5 * k]) * a.ftm2v;
      vcm[k][0] = s[5 * k + 1] / mass[k];
      vcm[k][1] = s[5 * k + 2] / mass[k];
      vcm[k][2] = s[5 * k + 3] / mass[k];
      const double t = 0.5 * mdp_dot3(vcm[k][0], vcm[k][0], vcm[k][1], vcm[k][1], vcm[k][2], vcm[k][2]) * mass[k];
      // FixHeat writes (ke + heat - t) / (ke - t).  The numerator is taken from the denominator here: under
      // -ffp-contract=fast the compiler fuses the products behind ke and t into the two differences in different ways, and
      // a source without flux would scale by 1 +- 1e-16; (den + 0) / den is 1 however den was rounded
      den[k] = ke - t;
      const double escale = (den[k] + a.heat[k]) / den[k];
      if (!(den[k] > 0.0) || !(escale >= 0.0)) bad = bad < 0 ? k : bad;
      else scale[k] = sqrt(escale);
    }
  }
  if (bad >= 0 && !latched) {
    st[kHeatErr] = 1.0;
    st[kHeatErr + 1] = (double) bad;
    st[bad * kHeatWords + kHeatErrStep] = a.step;
    latched = true;
  }
#pragma unroll
  for (int k = 0; k < kS; k++) {
    double *w = st + k * kHeatWords;
    if (a.mass) w[kHeatM] = mass[k];
    const bool apply = k < a.nsrc && ((a.due >> k) & 1) && !latched;
    const double sc = apply ? scale[k] : 1.0;
    w[kHeatS] = sc;
    w[kHeatVsub] = apply ? (sc - 1.0) * vcm[k][0] : 0.0;
    w[kHeatVsub + 1] = apply ? (sc - 1.0) * vcm[k][1] : 0.0;
    w[kHeatVsub + 2] = apply ? (sc - 1.0) * vcm[k][2] : 0.0;
    if (apply) {
      w[kHeatScale] = sc;
      w[kHeatVcm] = vcm[k][0];
      w[kHeatVcm + 1] = vcm[k][1];
      w[kHeatVcm + 2] = vcm[k][2];
      w[kHeatKe] = den[k];
      w[kHeatN] += 1.0;
    }
  }
}

// v = scale v - vsub on the atoms of every source, with the words the control workgroup left; every other atom is not
// written.  (fma: one rounding, the same in every build)
__global__ __launch_bounds__(256) void heat_apply_kernel(const int n, double *__restrict__ v, const HeatBits B,
                                                         const double *__restrict__ st, const MdpGroupArgs M)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int w = mdp_group_mask(M, i);
  if (!(w & B.any)) return;
  const int k = heat_src(B, w);
  double sc = st[kHeatS], sx = st[kHeatVsub], sy = st[kHeatVsub + 1], sz = st[kHeatVsub + 2];
#pragma unroll
  for (int b = 1; b < kS; b++) {
    sc = k == b ? st[b * kHeatWords + kHeatS] : sc;
    sx = k == b ? st[b * kHeatWords + kHeatVsub] : sx;
    sy = k == b ? st[b * kHeatWords + kHeatVsub + 1] : sy;
    sz = k == b ? st[b * kHeatWords + kHeatVsub + 2] : sz;
  }
  v[3 * (size_t) i] = fma(sc, v[3 * (size_t) i], -sx);
  v[3 * (size_t) i + 1] = fma(sc, v[3 * (size_t) i + 1], -sy);
  v[3 * (size_t) i + 2] = fma(sc, v[3 * (size_t) i + 2], -sz);
}

// the counts of a set-up or a mask upload: [0] atoms in more than one source, [1] source atoms outside the integrate
// group gbit (0: every atom is inside), [2 + k] atoms of source k
__global__ void heat_count_kernel(const int n, const int *__restrict__ mask, const HeatBits B, const int gbit, int *__restrict__ count)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int m = mask[i];
  if (!(m & B.any)) return;
  int in = 0;
#pragma unroll
  for (int k = 0; k < kS; k++)
    if (m & B.bit[k]) {
      in++;
      atomicAdd(count + 2 + k, 1);
    }
  if (in > 1) atomicAdd(count, 1);
  if (gbit && !(m & gbit)) atomicAdd(count + 1, 1);
}

HeatBits heat_bits(int nsrc, const int *bit)
{
  HeatBits B;
  for (int k = 0; k < nsrc; k++) {
    B.bit[k] = bit[k];
    B.any |= bit[k];
  }
  return B;
}

// counts the current mask for `nsrc` sources and refuses what a source cannot have (who: the call)
int heat_count(mdp_ctx *c, const char *who, int nsrc, const int *bit)
{
  MdpHeat &h = c->heat;
  MDP_HIP(c, h.count.reserve(2 + kS));
  const int zero[2 + kS] = {};
  MDP_TRY(mdp_write_small(c, h.count.p, zero, sizeof zero));
  const int n = c->mask_n;
  if (n) heat_count_kernel<<<nblk(n), 256, 0, c->stream>>>(n, c->mask.p, heat_bits(nsrc, bit), c->group_bit, h.count.p);
  MDP_HIP(c, hipGetLastError());
  int cnt[2 + kS];
  MDP_TRY(mdp_read_one(c, h.count.p, sizeof cnt, cnt));
  if (cnt[0])
    return mdp_fail(c, MDP_ESTATE, "%s: %d atoms are in more than one of the %d heat sources (mdp_heat_setup); the groups of the sources must be disjoint",
                    who, cnt[0], nsrc);
  if (cnt[1])
    return mdp_fail(c, MDP_ESTATE, "%s: %d atoms of the heat sources (mdp_heat_setup) are outside the integrate group (mdp_integrate_group)", who,
                    cnt[1]);
  for (int k = 0; k < nsrc; k++)
    if (!cnt[2 + k]) return mdp_fail(c, MDP_ESTATE, "%s: heat source %d has no atoms (group bit %d): its mass is 0", who, k, bit[k]);
  return MDP_OK;
}

} // namespace

int mdp_heat_mask(mdp_ctx *c, const char *who)
{
  MdpHeat &h = c->heat;
  if (!h.on) return MDP_OK;
  h.counted = false;
  h.mass_due = true;
  if (!mdp_mask_current(c)) return MDP_OK; // (the mask was withdrawn: the next pass says so)
  MDP_TRY(heat_count(c, who, h.nsrc, h.bit));
  h.counted = true;
  return MDP_OK;
}

int mdp_heat_pass(mdp_ctx *c)
{
  MdpHeat &h = c->heat;
  if (!h.on || !h.started) return MDP_OK; // (a final half before the run's first initial half belongs to the run before)
  int due = 0;
  for (int k = 0; k < h.nsrc; k++)
    if (h.step % h.cfg[k].nevery == 0) due |= 1 << k;
  if (!due) return MDP_OK;
  if (!mdp_mask_current(c))
    return mdp_fail(c, MDP_ESTATE, "%d heat sources are on (mdp_heat_setup) but no mask covers the current atoms (%s)", h.nsrc,
                    c->md ? "mdp_md_set_mask" : "mdp_hnve_set_mask after mdp_set_atoms_host");
  if (!h.counted) { // (a group call after the mask: counted once, here)
    MDP_TRY(heat_count(c, "integrate", h.nsrc, h.bit));
    h.counted = true;
  }
  const int n = c->nlocal;
  if (!n) return MDP_OK;
  const int nb = nblk(n), nbs = nblk(n, 256 * kHeatPer);
  MDP_HIP(c, h.part.reserve((size_t) kHeatW * nbs));
  const MdpStep s = mdp_step(c);
  const HeatBits B = heat_bits(h.nsrc, h.bit);
  const MdpGroupArgs M = mdp_mask_args(c);
  HeatCtl a;
  for (int k = 0; k < h.nsrc; k++) {
    a.heat[k] = h.cfg[k].eflux * h.cfg[k].nevery * s.dt * s.ftm2v;
    a.kefac[k] = 0.5 * h.cfg[k].mvv2e;
  }
  a.ftm2v = s.ftm2v;
  a.step = (double) h.step;
  a.due = due;
  a.nsrc = h.nsrc;
  a.mass = h.mass_due ? 1 : 0;
  heat_sums_kernel<<<nbs, 256, 0, c->stream>>>(n, c->rmass.p, c->v.p, B, h.part.p, M);
  heat_control_kernel<<<1, 256, 0, c->stream>>>(h.part.p, nbs, a, h.st.p);
  heat_apply_kernel<<<nb, 256, 0, c->stream>>>(n, c->v.p, B, h.st.p, M);
  MDP_HIP(c, hipGetLastError());
  h.mass_due = false;
  return MDP_OK;
}

// behind a wait for the stream: the error the control workgroup latched, if any
int mdp_heat_check(mdp_ctx *c)
{
  MdpHeat &h = c->heat;
  if (!h.on) return MDP_OK;
  double e[2];
  MDP_TRY(mdp_read_one(c, h.st.p + kHeatErr, sizeof e, e));
  if (e[0] == 0.0) return MDP_OK;
  const int k = (int) e[1];
  double step = -1.0;
  MDP_TRY(mdp_read_one(c, h.st.p + k * kHeatWords + kHeatErrStep, sizeof step, &step));
  return mdp_fail(c, MDP_ESTATE, "fix heat kinetic energy went negative (source %d, step %lld)", k, (long long) step);
}

extern "C" {

int mdp_heat_setup(mdp_ctx *c, int nsrc, const mdp_heat_config *cfg, const int *groupbit)
{
  if (!c || !cfg || !groupbit) return MDP_EINVAL;
  if (nsrc < 1 || nsrc > kS) return mdp_fail(c, MDP_EINVAL, "mdp_heat_setup: %d sources; a context takes 1 to %d", nsrc, kS);
  for (int k = 0; k < nsrc; k++) {
    if (!groupbit[k]) return mdp_fail(c, MDP_EINVAL, "mdp_heat_setup: source %d has group bit 0; every source acts on a group of its own", k);
    for (int j = 0; j < k; j++)
      if (groupbit[j] & groupbit[k])
        return mdp_fail(c, MDP_EINVAL, "mdp_heat_setup: sources %d and %d share the group bit %d", j, k, groupbit[j] & groupbit[k]);
    if (cfg[k].nevery < 1) return mdp_fail(c, MDP_EINVAL, "mdp_heat_setup: source %d: nevery must be >= 1", k);
    if (!std::isfinite(cfg[k].eflux)) return mdp_fail(c, MDP_EINVAL, "mdp_heat_setup: source %d: eflux must be finite", k);
    if (!(cfg[k].mvv2e > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_heat_setup: source %d: mvv2e must be > 0", k);
  }
  if (c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup: a minimisation (mdp_fire_setup) is on; mdp_fire_off first");
  if (c->nhc.on) return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup: the Nose-Hoover chain (mdp_nhc_setup) is on; heat sources run without a thermostat");
  MDP_TRY(mdp_refuse_if_on(c, "mdp_heat_setup", kRefuseOffFirst));
  if (c->lgv.on)
    return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup: the Langevin thermostat (mdp_langevin_setup) is on; heat sources run without a thermostat");
  if (c->dd.on && c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup: heat sources run on one rank only (this context is a brick of %d ranks)", c->dd.G.nranks);
  if (!c->md && !c->hn_on) return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup: no integrator on the context (mdp_md_setup or mdp_hnve_setup)");
  MDP_HIP(c, hipSetDevice(c->device));
  MdpHeat &h = c->heat;
  if (c->md) { // a final half the host deferred belongs to the run before: it completes now, without heat
    h.on = false;
    MDP_TRY(mdp_md_flush_final(c));
  }
  if (!mdp_mask_current(c))
    return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup: no mask covers the current atoms (%s)",
                    c->md ? "mdp_md_set_mask" : "mdp_hnve_set_mask after mdp_set_atoms_host");
  MDP_TRY(heat_count(c, "mdp_heat_setup", nsrc, groupbit));
  MDP_HIP(c, h.st.reserve(kHeatTotal));
  double st[kHeatTotal] = {};
  for (int k = 0; k < kS; k++) {
    st[k * kHeatWords + kHeatScale] = st[k * kHeatWords + kHeatS] = 1.0;
    st[k * kHeatWords + kHeatErrStep] = -1.0;
  }
  MDP_TRY(mdp_write_small(c, h.st.p, st, sizeof st));
  h.nsrc = nsrc;
  for (int k = 0; k < kS; k++) {
    h.bit[k] = k < nsrc ? groupbit[k] : 0;
    if (k < nsrc) h.cfg[k] = cfg[k];
  }
  h.counted = true;
  h.mass_due = true;
  h.step = 0;
  h.started = false;
  h.on = true;
  return MDP_OK;
}

int mdp_heat_run(mdp_ctx *c, long long first)
{
  if (!c) return MDP_EINVAL;
  MdpHeat &h = c->heat;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup not called");
  if (c->md) { // a final half the host deferred belongs to the run before: it completes now, without heat
    h.started = false;
    MDP_TRY(mdp_md_flush_final(c));
  }
  h.step = first;
  h.started = false;
  return MDP_OK;
}

int mdp_heat_state(mdp_ctx *c, int src, double *out)
{
  if (!c || !out) return MDP_EINVAL;
  const MdpHeat &h = c->heat;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_heat_setup not called");
  if (src < 0 || src >= h.nsrc) return mdp_fail(c, MDP_EINVAL, "mdp_heat_state: source index %d out of range (%d sources are on)", src, h.nsrc);
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(mdp_md_flush_final(c)); // (the application of the finished step)
  MDP_TRY(mdp_read_one(c, h.st.p + src * kHeatWords, sizeof(double) * MDP_HEAT_STATE_LEN, out));
  return mdp_heat_check(c);
}

int mdp_heat_off(mdp_ctx *c)
{
  if (!c) return MDP_EINVAL;
  // a deferred final half of the last heated step completes with its heat pass before plain NVE takes over
  if (c->heat.on && c->md) MDP_TRY(mdp_md_flush_final(c));
  c->heat.on = false;
  return MDP_OK;
}

} // extern "C"
