/* ------------------------------------------------------------------------------------------------
   compute heatflux/mdp -- see compute_heatflux_mdp.h.  What runs where:
     constructor        the arguments (refused here: an unknown or empty group, anything behind the style); the flags
                        that make LAMMPS tally per-atom energy and virial on the steps the compute is due
     init()             the one fix nve/mdp (or nvt/mdp) found through modify, in bricks mode (refused: none, the
                        host-linked mode -- there the tallies reach the host, and compute heat/flux is right)
     compute_vector()   the run's context through Fix::extract("mdp_steps_ctx"); mdp_heatflux_sums on this rank's brick
                        and MPI_Allreduce (the sums and the count of ranks that
                        were refused).  The library refuses a step that was not opened with per-atom tallies, and an
                        aeam brick whose angular centres reach remote ghosts; its text goes to error->all
-------------------------------------------------------------------------------------------------- */
#include "compute_heatflux_mdp.h"

#include "error.h"
#include "fix.h"
#include "group.h"
#include "modify.h"
#include "update.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

ComputeHeatFluxMDP::ComputeHeatFluxMDP(LAMMPS *lmp, int narg, char **arg) : Compute(lmp, narg, arg)
{
  const std::string head = "Illegal compute heatflux/mdp command: ";
  if (narg < 3) error->all(FLERR, head + "compute ID GROUP heatflux/mdp");
  if (igroup < 0)
    error->all(FLERR, std::string("Compute heatflux/mdp requires group all or a group defined by the group command: could not find compute group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Compute heatflux/mdp: group ") + arg[1] + " is empty: there is no atom to sum over");
  if (narg > 3) error->all(FLERR, head + "unknown keyword " + arg[3] + " (the compute takes none)");
  vector_flag = 1;
  size_vector = 6;
  extvector = 1;
  peatomflag = 1;    // Integrate::ev_set: per-atom energy ...
  pressatomflag = 1; // ... and per-atom virial on the steps this compute is due,
  timeflag = 1;      // which thermo and fix ave/time announce (Modify::addstep_compute)
  vector = out6;
  for (int k = 0; k < 6; k++) out6[k] = 0.0;
}

ComputeHeatFluxMDP::~ComputeHeatFluxMDP() {}

// the one time integrator of this plugin family: fix nve/mdp, or fix nvt/mdp that is built on it
Fix *ComputeHeatFluxMDP::integrator() const
{
  Fix *found = nullptr;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "nve/mdp") != 0 && strcmp(f->style, "nvt/mdp") != 0) continue;
    if (found) error->all(FLERR, std::string("Compute heatflux/mdp: fixes ") + found->id + " and " + f->id + " both integrate on the device; it reads one run's context");
    found = f;
  }
  return found;
}

void ComputeHeatFluxMDP::init()
{
  Fix *nve = integrator();
  if (!nve) error->all(FLERR, "Compute heatflux/mdp requires fix nve/mdp (or fix nvt/mdp) with bricks yes as the time integrator");
  int dim = 0;
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks", dim));
  if (!bricks || !nve->extract("mdp_steps_ctx", dim)) error->all(FLERR, std::string("Compute heatflux/mdp: fix ") + nve->id + " does not expose its run's context");
  if (!*bricks)
    error->all(FLERR, std::string("Compute heatflux/mdp: fix ") + nve->id + " runs in the host-linked mode, where the per-atom tallies reach the host: use compute heat/flux with ke/atom, pe/atom and stress/atom (or run the fix with bricks yes)");
}

void ComputeHeatFluxMDP::compute_vector()
{
  invoked_vector = update->ntimestep;
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **slot = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_steps_ctx", dim)) : nullptr;
  mdp_ctx *c = slot ? *slot : nullptr;
  if (!c) error->all(FLERR, "Compute heatflux/mdp: no run of fix nve/mdp is under way; the atoms are on the device only during one");
  // a refusal of the library -- a step without per-atom tallies, aeam centres that reach remote ghosts -- may come from one
  // rank's brick only: the count of refusals travels with the sums, so that every rank stops together
  double s[9], tot[9];
  const int rc = mdp_heatflux_sums(c, igroup > 0 ? groupbit : 0, s);
  if (rc != MDP_OK)
    for (int k = 0; k < 8; k++) s[k] = 0.0;
  s[8] = rc != MDP_OK ? 1.0 : 0.0;
  MPI_Allreduce(s, tot, 9, MPI_DOUBLE, MPI_SUM, world);
  if (tot[8] > 0.0)
    error->all(FLERR, std::string("Compute heatflux/mdp: ") + (rc != MDP_OK ? mdp_last_error(c) : "the brick of another rank refused the read"));
  for (int d = 0; d < 3; d++) {
    out6[d] = tot[d] + tot[3 + d];
    out6[3 + d] = tot[d];
  }
}
