/* ------------------------------------------------------------------------------------------------
   compute profile/mdp -- see compute_profile_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: no dimension, a dimension named twice, N
                        that is not a whole number >= 1, more than MDP_PROFILE_MAXBINS rows, an unknown keyword, a bad com
                        value, an unknown or empty group)
     init()             the one fix nve/mdp (or nvt/mdp) found through modify, in bricks mode (refused: none, the
                        host-linked mode -- there the host's atom->x and atom->v are current, and the chunk computes are right)
     compute_array()    the run's context through Fix::extract("mdp_steps_ctx"); the bins go up once per context
                        (mdp_profile_setup; mdp_profile_info tells whether they are still there); this rank's range, the
                        global maximum, the exponents (mdp_profile_exponent), this rank's integer table, its exact sum
                        over the ranks, the normalisation.  The mini-host's MPI subset has one reduction, MPI_SUM of
                        MPI_DOUBLE: the maximum is taken over per-rank slots of a summed vector of zeros, and a 64-bit
                        integer travels as q >> 31 and q & (2^31 - 1), whole numbers whose sums stay below 2^53.
-------------------------------------------------------------------------------------------------- */
#include "compute_profile_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "fix.h"
#include "force.h"
#include "group.h"
#include "modify.h"
#include "update.h"

#include <cmath>
#include <cstring>
#include <string>

using namespace LAMMPS_NS;

ComputeProfileMDP::ComputeProfileMDP(LAMMPS *lmp, int narg, char **arg)
    : Compute(lmp, narg, arg), ndim(0), comflag(0), nrows(1), sent_to(nullptr), sent_serial(0)
{
  const std::string head = "Illegal compute profile/mdp command: ";
  const std::string usage = "compute ID GROUP profile/mdp dim N [dim N [dim N]] [com yes|no], dim = x | y | z";
  if (igroup < 0)
    error->all(FLERR, std::string("Compute profile/mdp requires group all or a group defined by the group command: could not find compute group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Compute profile/mdp: group ") + arg[1] + " is empty: there is no atom to bin");
  for (int k = 0; k < 3; k++) {
    dim[k] = 0;
    nbin[k] = 1;
  }
  int iarg = 3;
  while (iarg < narg) {
    const std::string key = arg[iarg];
    if (key == "x" || key == "y" || key == "z") {
      const int d = key[0] - 'x';
      for (int k = 0; k < ndim; k++)
        if (dim[k] == d) error->all(FLERR, head + "dimension " + key + " is named twice");
      if (iarg + 1 >= narg) error->all(FLERR, head + "dimension " + key + " needs a number of bins");
      long long n = 0;
      if (!mdp_whole(arg[iarg + 1], n) || n < 1) error->all(FLERR, head + "N must be a whole number >= 1, not " + arg[iarg + 1]);
      if (n > MDP_PROFILE_MAXBINS || nrows * n > MDP_PROFILE_MAXBINS)
        error->all(FLERR, head + "more than " + std::to_string(MDP_PROFILE_MAXBINS) + " rows");
      dim[ndim] = d;
      nbin[ndim] = (int) n;
      nrows *= n;
      ndim++;
    } else if (key == "com") {
      if (iarg + 1 >= narg) error->all(FLERR, head + "com needs a value");
      comflag = mdp_yesno(error, head, key, arg[iarg + 1], true) ? 1 : 0;
    } else
      error->all(FLERR, head + "unknown keyword " + key);
    iarg += 2;
  }
  if (ndim == 0) error->all(FLERR, head + "no dimension: " + usage);
  if (atom->natoms < 1) error->all(FLERR, "Compute profile/mdp: there are no atoms");

  array_flag = 1;
  extarray = 0;
  size_array_rows = (int) nrows;
  size_array_cols = ndim + 7;
  values.assign((size_t) nrows * size_array_cols, 0.0);
  rows.resize((size_t) nrows);
  for (long long b = 0; b < nrows; b++) rows[(size_t) b] = values.data() + (size_t) b * size_array_cols;
  array = rows.data();
}

ComputeProfileMDP::~ComputeProfileMDP() {}

void ComputeProfileMDP::fail(mdp_ctx *c) { error->one(FLERR, std::string("Compute profile/mdp: ") + (c ? mdp_last_error(c) : "no device context")); }

// the one time integrator of this plugin family: fix nve/mdp, or fix nvt/mdp that is built on it
Fix *ComputeProfileMDP::integrator() const
{
  Fix *found = nullptr;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "nve/mdp") != 0 && strcmp(f->style, "nvt/mdp") != 0) continue;
    if (found) error->all(FLERR, std::string("Compute profile/mdp: fixes ") + found->id + " and " + f->id + " both integrate on the device; it reads one run's context");
    found = f;
  }
  return found;
}

void ComputeProfileMDP::init()
{
  Fix *nve = integrator();
  if (!nve) error->all(FLERR, "Compute profile/mdp requires fix nve/mdp (or fix nvt/mdp) with bricks yes as the time integrator");
  int dm = 0;
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks", dm));
  if (!bricks || !nve->extract("mdp_steps_ctx", dm)) error->all(FLERR, std::string("Compute profile/mdp: fix ") + nve->id + " does not expose its run's context");
  if (!*bricks)
    error->all(FLERR, std::string("Compute profile/mdp: fix ") + nve->id + " runs in the host-linked mode, where the host's atom->x and atom->v are current: use compute chunk/atom with fix ave/chunk (or run the fix with bricks yes)");
  sent_to = nullptr; // a new run may bring a new context: the bins go up again
}

void ComputeProfileMDP::compute_array()
{
  invoked_array = update->ntimestep;
  Fix *nve = integrator();
  int dm = 0;
  mdp_ctx **slot = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_steps_ctx", dm)) : nullptr;
  mdp_ctx *c = slot ? *slot : nullptr;
  if (!c) error->all(FLERR, "Compute profile/mdp: no run of fix nve/mdp is under way; the atoms are on the device only during one");
  long long info[4] = {0, 0, 0, 0};
  if (mdp_profile_info(c, info) != MDP_OK) fail(c);
  if (c != sent_to || !info[0] || info[3] != sent_serial) { // once per context, unless another measurement took its place
    if (mdp_profile_setup(c, ndim, dim, nbin, igroup > 0 ? groupbit : 0) != MDP_OK) fail(c);
    if (mdp_profile_info(c, info) != MDP_OK) fail(c);
    sent_to = c;
    sent_serial = info[3];
  }
  constexpr int W = MDP_PROFILE_W;
  const int me = comm->me, np = comm->nprocs;

  // the global maximum of |t_k| through a sum: every rank fills its own slot of a vector of zeros
  double range[W];
  if (mdp_profile_range(c, range) != MDP_OK) fail(c);
  std::vector<double> slots((size_t) np * W, 0.0), slots_all((size_t) np * W, 0.0);
  for (int k = 0; k < W; k++) slots[(size_t) me * W + k] = range[k];
  MPI_Allreduce(slots.data(), slots_all.data(), np * W, MPI_DOUBLE, MPI_SUM, world);
  int ex[W];
  for (int k = 0; k < W; k++) {
    double r = 0.0;
    for (int p = 0; p < np; p++) r = slots_all[(size_t) p * W + k] > r ? slots_all[(size_t) p * W + k] : r;
    ex[k] = mdp_profile_exponent(r, (long long) atom->natoms);
  }

  // this rank's integer table, then its exact sum over the ranks: counts as doubles, a 64-bit sum as its two halves
  const size_t nr = (size_t) nrows, ns = nr * W;
  std::vector<long long> count(nr, 0), sums(ns, 0);
  if (mdp_profile_sums(c, ex, count.data(), sums.data()) != MDP_OK) fail(c);
  const long long lomask = (1ll << 31) - 1;
  const size_t piece = 65536; // the reduction goes in pieces: a megabyte of transient buffers whatever the number of rows
  std::vector<double> mine(3 * piece), all(3 * piece);
  for (size_t at = 0; at < ns; at += piece) {
    const size_t len = ns - at < piece ? ns - at : piece;
    for (size_t k = 0; k < len; k++) {
      const long long q = sums[at + k];
      mine[k] = (double) (q >> 31);
      mine[len + k] = (double) (q & lomask);
    }
    MPI_Allreduce(mine.data(), all.data(), (int) (2 * len), MPI_DOUBLE, MPI_SUM, world);
    for (size_t k = 0; k < len; k++) sums[at + k] = (llrint(all[k]) << 31) + llrint(all[len + k]);
  }
  for (size_t at = 0; at < nr; at += piece) {
    const size_t len = nr - at < piece ? nr - at : piece;
    for (size_t k = 0; k < len; k++) mine[k] = (double) count[at + k];
    MPI_Allreduce(mine.data(), all.data(), (int) len, MPI_DOUBLE, MPI_SUM, world);
    for (size_t k = 0; k < len; k++) count[at + k] = llrint(all[k]);
  }

  // the normalisation (host/resident.py profile_normalise is the same arithmetic)
  const double vbin = domain->xprd * domain->yprd * domain->zprd / (double) nrows;
  const double mvv2e = force->mvv2e, boltz = force->boltz, mv2d = force->mv2d;
  for (size_t b = 0; b < nr; b++) {
    double *row = array[b];
    size_t rem = b;
    for (int k = ndim - 1; k >= 0; k--) { // the first named dimension slowest
      row[k] = ((double) (rem % (size_t) nbin[k]) + 0.5) / nbin[k];
      rem /= (size_t) nbin[k];
    }
    double t[W];
    for (int k = 0; k < W; k++) t[k] = ldexp((double) sums[b * W + k], -ex[k]);
    const double n = (double) count[b];
    double *val = row + ndim;
    val[0] = n;
    val[1] = n / vbin;
    if (count[b] <= 0) {
      for (int k = 2; k < 7; k++) val[k] = 0.0;
      continue;
    }
    const double msum = t[0] > 0.0 ? t[0] : 1.0;
    double kin = t[4];
    if (comflag) kin -= (t[1] * t[1] + t[2] * t[2] + t[3] * t[3]) / msum;
    val[2] = mv2d * t[0] / vbin;
    val[3] = mvv2e * kin / (3.0 * n * boltz);
    for (int k = 0; k < 3; k++) val[4 + k] = t[1 + k] / msum;
  }
}
