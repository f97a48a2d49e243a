/* ------------------------------------------------------------------------------------------------
   compute profile/mdp -- see compute_profile_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: no dimension, a dimension named twice, N
                        that is not a whole number >= 1, more than MDP_PROFILE_MAXBINS rows, an unknown keyword, a bad com
                        value)
     init()             bricks mode (the host-linked mode: there the host's atom->x and atom->v are current, and the chunk
                        computes are right)
     compute_array()    the bins go up once per context and run (mdp_profile_setup); this rank's range, the global
                        maximum, the exponents (mdp_profile_exponent), this rank's integer table, its exact sum over the
                        ranks (sum_whole), the normalisation.  The mini-host's MPI subset has one reduction, MPI_SUM of
                        MPI_DOUBLE: the maximum is taken over per-rank slots of a summed vector of zeros.
   The group refusals, the integrator, the run's context, the once-per-context protocol and the exact sum: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_profile_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "update.h"

#include <cmath>
#include <string>

using namespace LAMMPS_NS;

ComputeProfileMDP::ComputeProfileMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "profile/mdp", "there is no atom to bin"), ndim(0), comflag(0), nrows(1)
{
  const std::string usage = "compute ID GROUP profile/mdp dim N [dim N [dim N]] [com yes|no], dim = x | y | z";
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

  global_array(nrows, ndim + 7);
}

ComputeProfileMDP::~ComputeProfileMDP() {}

void ComputeProfileMDP::init()
{
  require_bricks("where the host's atom->x and atom->v are current: use compute chunk/atom with fix ave/chunk (or run the fix with bricks yes)");
  forget(); // a new run may bring a new context: the bins go up again
}

void ComputeProfileMDP::compute_array()
{
  invoked_array = update->ntimestep;
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_profile_info)) {
    if (mdp_profile_setup(c, ndim, dim, nbin, gbit()) != MDP_OK) fail(c);
    record(c, mdp_profile_info);
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

  // this rank's integer table, then its exact sum over the ranks
  const size_t nr = (size_t) nrows, ns = nr * W;
  std::vector<long long> count(nr, 0), sums(ns, 0);
  if (mdp_profile_sums(c, ex, count.data(), sums.data()) != MDP_OK) fail(c);
  sum_whole(sums.data(), ns);
  sum_whole(count.data(), nr);

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
