/* ------------------------------------------------------------------------------------------------
   compute heatflux/mdp -- see compute_heatflux_mdp.h.  What runs where:
     constructor        the arguments (refused here: anything behind the style); the flags that make LAMMPS tally
                        per-atom energy and virial on the steps the compute is due
     init()             bricks mode (the host-linked mode: there the tallies reach the host, and compute heat/flux is right)
     compute_vector()   mdp_heatflux_sums on this rank's brick and MPI_Allreduce (the sums and the count of ranks that
                        were refused).  The library refuses a step that was not opened with per-atom tallies, and an
                        aeam brick whose angular centres reach remote ghosts; its text goes to error->all
   The group refusals, the integrator and the run's context: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_heatflux_mdp.h"

#include "error.h"
#include "update.h"

#include <string>

using namespace LAMMPS_NS;

ComputeHeatFluxMDP::ComputeHeatFluxMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "heatflux/mdp", "there is no atom to sum over")
{
  if (narg < 3) error->all(FLERR, head + "compute ID GROUP heatflux/mdp");
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

void ComputeHeatFluxMDP::init()
{
  require_bricks("where the per-atom tallies reach the host: use compute heat/flux with ke/atom, pe/atom and stress/atom (or run the fix with bricks yes)");
}

void ComputeHeatFluxMDP::compute_vector()
{
  invoked_vector = update->ntimestep;
  mdp_ctx *c = run_context();
  // a refusal of the library -- a step without per-atom tallies, aeam centres that reach remote ghosts -- may come from one
  // rank's brick only: the count of refusals travels with the sums, so that every rank stops together
  double s[9], tot[9];
  const int rc = mdp_heatflux_sums(c, gbit(), s);
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
