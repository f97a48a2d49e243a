/* ------------------------------------------------------------------------------------------------
   compute cna/atom/mdp -- see compute_cna_atom_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: no Rc, a bad or non-positive Rc, anything
                        behind it)
     init()             bricks mode (the host-linked mode: there the host's atom->x and neighbour list are current, and compute
                        cna/atom is right); Rc against the pair style's cutforce
     compute_peratom()  the setup goes up once per context and run (mdp_cna_setup); mdp_cna_read on this rank's brick, into
                        vector_atom behind the check of the tags (compute_mdp.h, read_peratom); then the census of that read
                        (mdp_cna_counts), summed exactly over the ranks, and the warning about atoms with more than 16
                        neighbours on the rank that has them
     compute_vector()   the census of this step: compute_peratom() unless it has run on this step
   The group refusals, the integrator, the run's context and the once-per-context protocol: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_cna_atom_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "error.h"
#include "force.h"
#include "pair.h"
#include "update.h"

#include <string>

using namespace LAMMPS_NS;

ComputeCnaAtomMDP::ComputeCnaAtomMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "cna/atom/mdp", "there is no atom to look around"), cutoff(0.0)
{
  const std::string usage = "compute ID GROUP cna/atom/mdp Rc";
  if (narg < 4) error->all(FLERR, head + usage);
  cutoff = mdp_number(error, head, "Rc", arg[3], true);
  if (!(cutoff > 0.0)) error->all(FLERR, head + "Rc must be > 0, not " + arg[3]);
  if (narg > 4) error->all(FLERR, head + "nothing follows Rc, not " + arg[4] + ": " + usage);
  if (atom->natoms < 1) error->all(FLERR, "Compute cna/atom/mdp: there are no atoms");
  if (!atom->tag_enable) error->all(FLERR, "Compute cna/atom/mdp requires atom IDs");
  peratom_columns(1);
  vector_flag = 1;
  size_vector = 5;
  extvector = 1;
  vector = census;
  for (int k = 0; k < 5; k++) census[k] = 0.0;
}

ComputeCnaAtomMDP::~ComputeCnaAtomMDP() {}

void ComputeCnaAtomMDP::init()
{
  require_bricks("where the host's atom->x and neighbour list are current: use compute cna/atom (or run the fix with bricks yes)");
  if (!force->pair) error->all(FLERR, "Compute cna/atom/mdp requires a pair style: its cutforce sets the ghost shell the neighbours come from");
  const double cutforce = force->pair->cutforce;
  if (cutoff > cutforce * (1.0 + 1e-12)) {
    char buf[320];
    snprintf(buf, sizeof buf, "Compute cna/atom/mdp: the cutoff %g is beyond the pair style's cutforce %.15g: the brick's ghost shell is cutforce + "
                              "skin wide as of the last reneighbouring, so only neighbours within cutforce are all present",
             cutoff, cutforce);
    error->all(FLERR, buf);
  }
  forget(); // a new run may bring a new context: the setup goes up again
}

void ComputeCnaAtomMDP::compute_peratom()
{
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_cna_info)) {
    if (mdp_cna_setup(c, cutoff, gbit()) != MDP_OK) fail(c);
    record(c, mdp_cna_info);
  }
  read_peratom(c, mdp_cna_read);
  long long mine[6], info[4];
  if (mdp_cna_counts(c, mine) != MDP_OK || mdp_cna_info(c, info) != MDP_OK) fail(c);
  if (info[2] > 0) error->warning(FLERR, "Too many neighbors in CNA for " + std::to_string(info[2]) + " atoms");
  sum_whole(mine, 6);
  for (int k = 0; k < 5; k++) census[k] = (double) mine[k + 1];
  invoked_vector = update->ntimestep;
}

void ComputeCnaAtomMDP::compute_vector()
{
  if (invoked_peratom != update->ntimestep) compute_peratom(); // (one read per step serves both)
  invoked_vector = update->ntimestep;
}
