/* ------------------------------------------------------------------------------------------------
   compute msd/mdp -- see compute_msd_mdp.h.  What runs where:
     constructor        the arguments (refused here: an unknown or empty group, average yes, an unknown keyword); the
                        origins: a zeroed [natoms][3] array filled at this rank's tags with x + h . image of the host's
                        atoms, summed over the ranks; the group's centre of mass there
     init()             the one fix nve/mdp (or nvt/mdp) found through modify, in bricks mode (refused: none, the
                        host-linked mode -- there the host keeps atom->image itself, and compute msd is right)
     compute_vector()   the run's context through Fix::extract("mdp_steps_ctx"); the origins go up once per context
                        (mdp_msd_setup; mdp_msd_info tells whether they are still there); mdp_msd_sums on this rank's
                        brick -- twice with com yes: the mass sums, then the pass with the shift -- and MPI_Allreduce
-------------------------------------------------------------------------------------------------- */
#include "compute_msd_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "fix.h"
#include "group.h"
#include "modify.h"
#include "update.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

ComputeMSDMDP::ComputeMSDMDP(LAMMPS *lmp, int narg, char **arg)
    : Compute(lmp, narg, arg), comflag(0), nall(0), sent_to(nullptr), sent_serial(0)
{
  const std::string head = "Illegal compute msd/mdp command: ";
  if (narg < 3) error->all(FLERR, head + "compute ID GROUP msd/mdp [com yes|no]");
  if (igroup < 0)
    error->all(FLERR, std::string("Compute msd/mdp requires group all or a group defined by the group command: could not find compute group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Compute msd/mdp: group ") + arg[1] + " is empty: there is no atom to measure");
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

void ComputeMSDMDP::fail(mdp_ctx *c) { error->one(FLERR, std::string("Compute msd/mdp: ") + (c ? mdp_last_error(c) : "no device context")); }

// the one time integrator of this plugin family: fix nve/mdp, or fix nvt/mdp that is built on it
Fix *ComputeMSDMDP::integrator() const
{
  Fix *found = nullptr;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "nve/mdp") != 0 && strcmp(f->style, "nvt/mdp") != 0) continue;
    if (found) error->all(FLERR, std::string("Compute msd/mdp: fixes ") + found->id + " and " + f->id + " both integrate on the device; it reads one run's context");
    found = f;
  }
  return found;
}

void ComputeMSDMDP::init()
{
  Fix *nve = integrator();
  if (!nve) error->all(FLERR, "Compute msd/mdp requires fix nve/mdp (or fix nvt/mdp) with bricks yes as the time integrator");
  int dim = 0;
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks", dim));
  if (!bricks || !nve->extract("mdp_steps_ctx", dim)) error->all(FLERR, std::string("Compute msd/mdp: fix ") + nve->id + " does not expose its run's context");
  if (!*bricks)
    error->all(FLERR, std::string("Compute msd/mdp: fix ") + nve->id + " runs in the host-linked mode, where the host keeps atom->image itself: use compute msd (or run the fix with bricks yes)");
}

void ComputeMSDMDP::compute_vector()
{
  invoked_vector = update->ntimestep;
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **slot = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_steps_ctx", dim)) : nullptr;
  mdp_ctx *c = slot ? *slot : nullptr;
  if (!c) error->all(FLERR, "Compute msd/mdp: no run of fix nve/mdp is under way; the atoms are on the device only during one");
  long long info[4] = {0, 0, 0, 0};
  if (mdp_msd_info(c, info) != MDP_OK) fail(c);
  if (c != sent_to || !info[0] || info[3] != sent_serial) { // once per context, unless another measurement took its place
    if (mdp_msd_setup(c, (int) nall, x0.data(), igroup > 0 ? groupbit : 0) != MDP_OK) fail(c);
    if (mdp_msd_info(c, info) != MDP_OK) fail(c);
    sent_to = c;
    sent_serial = info[3];
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
