/* ------------------------------------------------------------------------------------------------
   compute msd/mdp -- see compute_msd_mdp.h.  What runs where:
     constructor        the arguments (refused here: average yes, an unknown keyword); the origins: a zeroed [natoms][3]
                        array filled at this rank's tags with x + h . image of the host's atoms, summed over the ranks;
                        the group's centre of mass there
     init()             bricks mode (the host-linked mode: there the host keeps atom->image itself, and compute msd is right)
     compute_vector()   the origins go up once per context, not once per run (mdp_msd_setup); mdp_msd_sums on this rank's
                        brick -- twice with com yes: the mass sums, then the pass with the shift -- and MPI_Allreduce
   The group refusals, the integrator, the run's context and the once-per-context protocol: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_msd_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "update.h"

#include <string>

using namespace LAMMPS_NS;

ComputeMSDMDP::ComputeMSDMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "msd/mdp", "there is no atom to measure"), comflag(0), nall(0)
{
  if (narg < 3) error->all(FLERR, head + "compute ID GROUP msd/mdp [com yes|no]");
  for (int k = 3; k < narg; k += 2) {
    const std::string key = arg[k];
    if (key != "com" && key != "average") error->all(FLERR, head + "unknown keyword " + key);
    if (k + 1 >= narg) error->all(FLERR, head + key + " needs a value");
    const bool yes = mdp_yesno(error, head, key, arg[k + 1], true);
    if (key == "com") comflag = yes ? 1 : 0;
    else if (yes) error->all(FLERR, "Compute msd/mdp: average yes is not supported (the origins are fixed at the compute's definition)");
  }
  vector_flag = 1;
  size_vector = 4;
  extvector = 0;
  vector = out4;
  for (int k = 0; k < 4; k++) out4[k] = 0.0;

  // the origins: LAMMPS' Domain::unmap of every owned atom, at its tag; the other ranks fill in theirs
  nall = atom->natoms;
  if (nall < 1) error->all(FLERR, "Compute msd/mdp: there are no atoms");
  if (!atom->tag_enable) error->all(FLERR, "Compute msd/mdp requires atom IDs");
  const double *h = domain->h; // xprd, yprd, zprd, yz, xz, xy
  std::vector<double> mine((size_t) 3 * nall, 0.0);
  double cm[4] = {0.0, 0.0, 0.0, 0.0}, cmall[4];
  for (int i = 0; i < atom->nlocal; i++) {
    const bigint t = atom->tag[i];
    if (t < 1 || t > nall) error->one(FLERR, "Compute msd/mdp requires consecutive atom IDs 1 .. natoms");
    const imageint im = atom->image[i];
    const double ix = (double) ((im & IMGMASK) - IMGMAX), iy = (double) (((im >> IMGBITS) & IMGMASK) - IMGMAX),
                 iz = (double) ((im >> IMG2BITS) - IMGMAX);
    double *o = mine.data() + 3 * (size_t) (t - 1);
    o[0] = atom->x[i][0] + h[0] * ix + h[5] * iy + h[4] * iz;
    o[1] = atom->x[i][1] + h[1] * iy + h[3] * iz;
    o[2] = atom->x[i][2] + h[2] * iz;
    if (atom->mask[i] & groupbit) {
      const double m = atom->mass[atom->type[i]];
      for (int d = 0; d < 3; d++) cm[d] += m * o[d];
      cm[3] += m;
    }
  }
  x0.assign((size_t) 3 * nall, 0.0);
  MPI_Allreduce(mine.data(), x0.data(), (int) (3 * nall), MPI_DOUBLE, MPI_SUM, world);
  MPI_Allreduce(cm, cmall, 4, MPI_DOUBLE, MPI_SUM, world);
  for (int d = 0; d < 3; d++) cm0[d] = cmall[3] > 0.0 ? cmall[d] / cmall[3] : 0.0;
}

ComputeMSDMDP::~ComputeMSDMDP() {}

void ComputeMSDMDP::init() { require_bricks("where the host keeps atom->image itself: use compute msd (or run the fix with bricks yes)"); }

void ComputeMSDMDP::compute_vector()
{
  invoked_vector = update->ntimestep;
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_msd_info)) {
    if (mdp_msd_setup(c, (int) nall, x0.data(), gbit()) != MDP_OK) fail(c);
    record(c, mdp_msd_info);
  }
  double s[8], tot[8];
  const double *shift = nullptr;
  double sh[3];
  if (comflag) { // the mass sums first: cm(t), then the pass with shift = cm(t) - cm(0)
    if (mdp_msd_sums(c, nullptr, s) != MDP_OK) fail(c);
    MPI_Allreduce(s, tot, 8, MPI_DOUBLE, MPI_SUM, world);
    for (int d = 0; d < 3; d++) sh[d] = (tot[7] > 0.0 ? tot[4 + d] / tot[7] : 0.0) - cm0[d];
    shift = sh;
  }
  if (mdp_msd_sums(c, shift, s) != MDP_OK) fail(c);
  MPI_Allreduce(s, tot, 8, MPI_DOUBLE, MPI_SUM, world);
  for (int d = 0; d < 3; d++) out4[d] = tot[3] > 0.0 ? tot[d] / tot[3] : 0.0;
  out4[3] = out4[0] + out4[1] + out4[2];
}
