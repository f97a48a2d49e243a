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
// Several baths (mdp_langevin_baths, nbath > 1): bath k acts on the atoms of its group bit with its own table, target,
// seed, mean and tally.  The kernels read the mask once, pick the bath index by compare/select and take everything else
// from that index; the block sums carry one slot per bath.
// One code path serves both: every kernel, the argument struct (MdpLgvArgs) and mdp_lgv_open / _close are templates on the
// slot count NB, instantiated for 1 and for MDP_LANGEVIN_MAXBATH.  With NB = 1 the bath index is the constant 0, so the
// mask is not read for it and the selects fold away: one bath costs what it cost before there were several.
#include "mdp_common.h"

#include <cmath>

namespace {

constexpr int kB = MDP_LANGEVIN_MAXBATH;

// zero yes: part[3 (NB b + k) + j] = the sum over block b of the random parts fran_j of bath k's atoms (mdp_lgv_random)
// MASK: of the baths' atoms alone (MdpGroupArgs); the others add 0 and still reach the block sum.  Several baths always
// come with a mask
template <int NB, bool MASK>
__global__ __launch_bounds__(256) void lgv_zero_kernel(const int n, const MdpLgvArgs<NB> L, double *__restrict__ part,
                                                       const MdpGroupArgs M)
{
  static_assert(MASK || NB == 1, "several baths are told apart by the mask");
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool in = i < n;
  int k = 0;
  if constexpr (MASK)
    if (in) {
      const int m = mdp_group_mask(M, i);
      in = mdp_group_lgv(M, m);
      k = mdp_lgv_bath(L, m);
    }
  double rx = 0.0, ry = 0.0, rz = 0.0;
  if (in) mdp_lgv_random(L, i, k, rx, ry, rz);
  double r[3 * NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    r[3 * b] = k == b ? rx : 0.0;
    r[3 * b + 1] = k == b ? ry : 0.0;
    r[3 * b + 2] = k == b ? rz : 0.0;
  }
  mdp_block_sum_256<3 * NB>(r, part);
}

// what the two one-workgroup kernels below need of every bath (the slots beyond nbath have neither zero nor tally)
struct LgvBathSums {
  double natoms[kB] = {1.0, 1.0, 1.0, 1.0};
  int zero[kB] = {0, 0, 0, 0}, tally[kB] = {0, 0, 0, 0};
};

// zero yes: the mean of every zero yes bath, (the sum of its random parts) / ITS natoms, all components in one pass over
// the slots; the mean words of the other baths stay 0
template <int NB>
__global__ __launch_bounds__(256) void lgv_mean_kernel(const double *__restrict__ part, const int npart, const LgvBathSums S,
                                                       double *__restrict__ st)
{
  double s[3 * NB];
  mdp_slot_sum_256<3 * NB>(part, npart, s);
#pragma unroll
  for (int k = 0; k < 3 * NB; k++)
    if ((int) threadIdx.x == k && S.zero[k / 3]) st[(k / 3) * kLgvWords + kLgvMean + k % 3] = s[k] / S.natoms[k / 3];
}

// tally yes, for every bath that has a tally, from its slot of the partials: E = the fixed-order sum of the partials of
// f_L . v; the setup force starts the energy of the run at 0.5 E dt (FixLangevin::compute_scalar at beginstep), a step
// adds E dt (end_of_step)
template <int NB>
__global__ __launch_bounds__(256) void lgv_tally_kernel(const double *__restrict__ part, const int npart, const double dt,
                                                        const int setup, const LgvBathSums S, double *__restrict__ st)
{
  double e[NB];
  mdp_slot_sum_256<NB>(part, npart, e);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NB; k++)
      if (S.tally[k]) {
        double *b = st + k * kLgvWords;
        b[kLgvE] = setup ? 0.5 * e[k] * dt : b[kLgvE] + e[k] * dt;
        b[kLgvElast] = e[k];
      }
  }
}

// atoms of the mask that are in more than one of the baths
__global__ void lgv_overlap_kernel(const int n, const int *__restrict__ mask, const int b0, const int b1, const int b2,
                                   const int b3, int *__restrict__ count)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int m = mask[i];
  const int in = ((m & b0) != 0) + ((m & b1) != 0) + ((m & b2) != 0) + ((m & b3) != 0);
  if (in > 1) atomicAdd(count, 1);
}

double lgv_target(const MdpLangevin &h, const mdp_langevin_config &g, long long n)
{
  double delta = h.last == h.first ? 0.0 : (double) (n - h.first) / (double) (h.last - h.first);
  delta = delta < 0.0 ? 0.0 : (delta > 1.0 ? 1.0 : delta); // (steps beyond `last` hold Tstop: T never goes negative)
  return g.t_start + delta * (g.t_stop - g.t_start);
}

// the per-type factors of FixLangevin::init for this time step and unit system (rewritten when they change)
int lgv_tables(mdp_ctx *c)
{
  MdpLangevin &h = c->lgv;
  const MdpStep s = mdp_step(c);
  const double dt = s.dt, ftm2v = s.ftm2v, *mass = s.mass;
  if (h.tab_dt == dt && h.tab_ftm2v == ftm2v) return MDP_OK;
  for (int k = 0; k < h.nbath; k++) {
    const mdp_langevin_config &g = h.cfg[k];
    double tab[2 * 16] = {};
    for (int t = 1; t < 16; t++) {
      const double m = mass[t] > 0.0 ? mass[t] : 0.0;
      tab[t] = -m / g.t_period / ftm2v;
      tab[kLgvG2 + t] = sqrt(m) * sqrt(24.0 * g.boltz / g.t_period / dt / g.mvv2e) / ftm2v;
      tab[t] *= 1.0 / g.ratio[t];
      tab[kLgvG2 + t] *= 1.0 / sqrt(g.ratio[t]);
    }
    MDP_TRY(mdp_write_small(c, h.st.p + k * kLgvWords, tab, sizeof tab));
  }
  h.tab_dt = dt;
  h.tab_ftm2v = ftm2v;
  return MDP_OK;
}

LgvBathSums lgv_bath_sums(const MdpLangevin &h)
{
  LgvBathSums S;
  for (int k = 0; k < h.nbath; k++) {
    S.natoms[k] = (double) h.cfg[k].natoms;
    S.zero[k] = h.cfg[k].zero ? 1 : 0;
    S.tally[k] = h.cfg[k].tally ? 1 : 0;
  }
  return S;
}

// the count of lgv_overlap_kernel over the current mask, for `nbath` bits
int lgv_count_overlap(mdp_ctx *c, int nbath, const int *bit, int *count)
{
  MdpLangevin &h = c->lgv;
  MDP_HIP(c, h.overlap.reserve(1));
  const int zero = 0;
  MDP_TRY(mdp_write_small(c, h.overlap.p, &zero, sizeof zero));
  int b[kB] = {0, 0, 0, 0};
  for (int k = 0; k < nbath; k++) b[k] = bit[k];
  const int n = c->mask_n;
  if (n) lgv_overlap_kernel<<<nblk(n), 256, 0, c->stream>>>(n, c->mask.p, b[0], b[1], b[2], b[3], h.overlap.p);
  MDP_HIP(c, hipGetLastError());
  return mdp_read_one(c, h.overlap.p, sizeof(int), count);
}

// the argument errors of one thermostat's configuration; who: the call, and the bath where there are several
int lgv_check_config(mdp_ctx *c, const char *who, const mdp_langevin_config *cfg)
{
  if ((cfg->zero || cfg->tally) && c->dd.on && c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "%s: zero and tally run on one rank only (this context is a brick of %d ranks)", who,
                    c->dd.G.nranks);
  if (cfg->seed <= 0) return mdp_fail(c, MDP_EINVAL, "%s: the seed must be > 0", who);
  if (!(cfg->t_period > 0.0)) return mdp_fail(c, MDP_EINVAL, "%s: damp must be > 0", who);
  if (!(cfg->t_start >= 0.0) || !(cfg->t_stop >= 0.0)) return mdp_fail(c, MDP_EINVAL, "%s: Tstart and Tstop must be >= 0", who);
  for (int t = 1; t < 16; t++)
    if (!(cfg->ratio[t] > 0.0)) return mdp_fail(c, MDP_EINVAL, "%s: the scale ratio of type %d must be > 0", who, t);
  if (!(cfg->boltz > 0.0) || !(cfg->mvv2e > 0.0) || (cfg->zero && cfg->natoms < 1))
    return mdp_fail(c, MDP_EINVAL, "%s: boltz, mvv2e or natoms out of range", who);
  return MDP_OK;
}

// the energy a bath has taken out of its atoms up to the last full step, from its two words (0 without tally yes)
int lgv_read_tally(mdp_ctx *c, int bath, double *out)
{
  if (!c->lgv.cfg[bath].tally) {
    *out = 0.0;
    return MDP_OK;
  }
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(mdp_md_flush_final(c)); // (the energy of the finished step)
  double e[2];
  MDP_TRY(mdp_read_one(c, c->lgv.st.p + bath * kLgvWords + kLgvE, sizeof e, e));
  *out = -(e[0] - 0.5 * e[1] * mdp_step(c).dt); // FixLangevin::compute_scalar: back from mid-step to the last full step
  return MDP_OK;
}

} // namespace

int mdp_lgv_check_disjoint(mdp_ctx *c, const char *who)
{
  MdpLangevin &h = c->lgv;
  if (h.disjoint_checked) return MDP_OK;
  int count = 0;
  MDP_TRY(lgv_count_overlap(c, h.nbath, h.bit, &count));
  if (count)
    return mdp_fail(c, MDP_ESTATE, "%s: %d atoms are in more than one of the %d Langevin baths (mdp_langevin_baths); the groups of the baths must be disjoint",
                    who, count, h.nbath);
  h.disjoint_checked = true;
  return MDP_OK;
}

template <int NB> int mdp_lgv_open(mdp_ctx *c, bool with_final, bool initial, bool *apply, MdpLgvArgs<NB> *L)
{
  MdpLangevin &h = c->lgv;
  const int n = c->nlocal;
  const bool setup = initial && !with_final && h.need_setup;
  *apply = !initial || with_final || setup;
  if (*apply) {
    MDP_TRY(lgv_tables(c));
    const int nb = nblk(n);
    MDP_HIP(c, h.part.reserve((size_t) 4 * NB * nb + 4 * NB));
    L->tag = c->tag.p;
    L->type = c->type.p;
    L->perm = !c->md && c->host_sort ? c->host_perm.p : nullptr; // host mode: tags and types are in the host's order
    L->st = h.st.p;
    for (int k = 0; k < NB && k < h.nbath; k++) {
      L->tsqrt[k] = sqrt(lgv_target(h, h.cfg[k], h.step));
      L->seed[k] = (unsigned) h.cfg[k].seed;
      if constexpr (NB > 1) L->bit[k] = h.bit[k];
    }
    L->lo = (unsigned) (unsigned long long) h.step;
    L->hi = (unsigned) ((unsigned long long) h.step >> 32);
    L->phase = setup ? 1u : 0u;
    L->mean = h.any_zero ? h.st.p + kLgvMean : nullptr;
    L->part = h.any_tally ? h.part.p + (size_t) 3 * NB * nb : nullptr;
    if (h.any_zero) {
      bool masked = false;
      MdpGroupArgs M;
      MDP_TRY(mdp_group_args(c, &masked, &M));
      if (n && masked) lgv_zero_kernel<NB, true><<<nb, 256, 0, c->stream>>>(n, *L, h.part.p, M);
      if constexpr (NB == 1) // (several baths always come with a mask: mdp_group_args)
        if (n && !masked) lgv_zero_kernel<1, false><<<nb, 256, 0, c->stream>>>(n, *L, h.part.p, M);
      lgv_mean_kernel<NB><<<1, 256, 0, c->stream>>>(h.part.p, n ? nb : 0, lgv_bath_sums(h), h.st.p);
      MDP_HIP(c, hipGetLastError());
    }
  }
  if (initial) {
    h.need_setup = false;
    h.step++;
  }
  return MDP_OK;
}

template <int NB> int mdp_lgv_close(mdp_ctx *c, const MdpLgvArgs<NB> &L)
{
  if (!L.part) return MDP_OK;
  lgv_tally_kernel<NB><<<1, 256, 0, c->stream>>>(L.part, c->nlocal ? nblk(c->nlocal) : 0, mdp_step(c).dt, L.phase == 1u ? 1 : 0,
                                                 lgv_bath_sums(c->lgv), c->lgv.st.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}

template int mdp_lgv_open<1>(mdp_ctx *, bool, bool, bool *, MdpLgvArgs<1> *);
template int mdp_lgv_open<kB>(mdp_ctx *, bool, bool, bool *, MdpLgvArgs<kB> *);
template int mdp_lgv_close<1>(mdp_ctx *, const MdpLgvArgs<1> &);
template int mdp_lgv_close<kB>(mdp_ctx *, const MdpLgvArgs<kB> &);

extern "C" {

int mdp_langevin_setup(mdp_ctx *c, const mdp_langevin_config *cfg)
{
  if (!c || !cfg) return MDP_EINVAL;
  if (c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup: a minimisation (mdp_fire_setup) is on; mdp_fire_off first");
  if (c->heat.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup: heat sources (mdp_heat_setup) are on; mdp_heat_off first");
  if (c->nhc.on)
    return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup: the Nose-Hoover chain (mdp_nhc_setup) is on; one thermostat per context");
  MDP_TRY(lgv_check_config(c, "mdp_langevin_setup", cfg));
  MDP_HIP(c, hipSetDevice(c->device));
  MdpLangevin &h = c->lgv;
  MDP_HIP(c, h.st.reserve(kLgvWords));
  double zero[kLgvWords] = {};
  MDP_TRY(mdp_write_small(c, h.st.p, zero, sizeof zero));
  h.cfg[0] = *cfg; // one bath, on the group of mdp_langevin_group (mdp_langevin_baths sets what several need)
  h.nbath = 1;
  for (int k = 0; k < kB; k++) h.bit[k] = 0;
  h.any_zero = cfg->zero;
  h.any_tally = cfg->tally;
  h.tab_dt = h.tab_ftm2v = 0.0; // (the factors are computed by the first kernel that needs them)
  h.first = h.last = h.step = 0;
  h.need_setup = true;
  h.on = true;
  return MDP_OK;
}

int mdp_langevin_baths(mdp_ctx *c, int nbath, const mdp_langevin_config *cfg, const int *groupbit)
{
  if (!c || !cfg || !groupbit) return MDP_EINVAL;
  if (nbath < 1 || nbath > MDP_LANGEVIN_MAXBATH)
    return mdp_fail(c, MDP_EINVAL, "mdp_langevin_baths: %d baths; a context takes 1 to %d", nbath, MDP_LANGEVIN_MAXBATH);
  if (c->fire.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_baths: a minimisation (mdp_fire_setup) is on; mdp_fire_off first");
  if (c->heat.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_baths: heat sources (mdp_heat_setup) are on; mdp_heat_off first");
  if (c->nhc.on)
    return mdp_fail(c, MDP_ESTATE, "mdp_langevin_baths: the Nose-Hoover chain (mdp_nhc_setup) is on; one kind of thermostat per context");
  for (int k = 0; k < nbath; k++) {
    if (!groupbit[k]) return mdp_fail(c, MDP_EINVAL, "mdp_langevin_baths: bath %d has group bit 0; every bath acts on a group of its own", k);
    for (int j = 0; j < k; j++)
      if (groupbit[j] & groupbit[k])
        return mdp_fail(c, MDP_EINVAL, "mdp_langevin_baths: baths %d and %d share the group bit %d", j, k, groupbit[j] & groupbit[k]);
  }
  for (int k = 0; k < nbath; k++) {
    char who[48];
    snprintf(who, sizeof who, "mdp_langevin_baths: bath %d", k);
    MDP_TRY(lgv_check_config(c, who, cfg + k));
  }
  if (c->md && c->lgv.on) MDP_TRY(mdp_md_flush_final(c)); // (a deferred final half belongs to the set-up it ran with)
  if (nbath == 1) { // the one thermostat, through the calls that have always set it up
    MDP_TRY(mdp_langevin_setup(c, cfg));
    return mdp_langevin_group(c, groupbit[0]);
  }
  MDP_HIP(c, hipSetDevice(c->device));
  if (c->md) MDP_TRY(mdp_md_flush_final(c));
  MdpLangevin &h = c->lgv;
  if (c->mask_set && c->mask_n == c->nlocal) {
    int count = 0;
    MDP_TRY(lgv_count_overlap(c, nbath, groupbit, &count));
    if (count)
      return mdp_fail(c, MDP_ESTATE, "mdp_langevin_baths: %d atoms are in more than one of the %d Langevin baths (mdp_langevin_baths); the groups of the baths must be disjoint",
                      count, nbath);
  }
  MDP_HIP(c, h.st.reserve((size_t) kB * kLgvWords));
  double zero[kB * kLgvWords] = {};
  MDP_TRY(mdp_write_small(c, h.st.p, zero, sizeof zero));
  h.nbath = nbath;
  h.any_zero = h.any_tally = false;
  for (int k = 0; k < kB; k++) {
    h.bit[k] = k < nbath ? groupbit[k] : 0;
    if (k < nbath) {
      h.cfg[k] = cfg[k];
      h.any_zero = h.any_zero || cfg[k].zero;
      h.any_tally = h.any_tally || cfg[k].tally;
    }
  }
  h.disjoint_checked = c->mask_set && c->mask_n == c->nlocal;
  c->lgv_bit = 0;
  h.tab_dt = h.tab_ftm2v = 0.0;
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
  const MdpLangevin &h = c->lgv;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup not called");
  if (h.nbath == 1) return lgv_read_tally(c, 0, out); // (as read: 0.0 + in front of it would lose the sign of a -0.0)
  double sum = 0.0; // the sum over the baths in bath order
  for (int k = 0; k < h.nbath; k++) {
    double e = 0.0;
    MDP_TRY(lgv_read_tally(c, k, &e));
    sum += e;
  }
  *out = sum;
  return MDP_OK;
}

int mdp_langevin_tally_bath(mdp_ctx *c, int bath, double *out)
{
  if (!c || !out) return MDP_EINVAL;
  const MdpLangevin &h = c->lgv;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_langevin_setup not called");
  if (bath < 0 || bath >= h.nbath)
    return mdp_fail(c, MDP_EINVAL, "mdp_langevin_tally_bath: bath index %d out of range (%d baths are on)", bath, h.nbath);
  return lgv_read_tally(c, bath, out);
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
