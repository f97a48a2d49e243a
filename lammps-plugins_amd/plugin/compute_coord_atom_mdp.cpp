/* ------------------------------------------------------------------------------------------------
   compute coord/atom/mdp -- see compute_coord_atom_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: no cutoff keyword, the orientorder form, the
                        group keyword, a bad or non-positive Rc, a type range outside 1 .. ntypes, more than 32 columns)
     init()             bricks mode (the host-linked mode: there the host's atom->x and neighbour list are current, and compute
                        coord/atom is right); Rc against the pair style's cutforce
     compute_peratom()  the setup goes up once per context and run (mdp_coord_setup); mdp_coord_read on this rank's brick, into
                        vector_atom / array_atom behind the check of the tags (compute_mdp.h, read_peratom)
   The group refusals, the integrator, the run's context and the once-per-context protocol: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_coord_atom_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "error.h"
#include "force.h"
#include "pair.h"

#include <string>

using namespace LAMMPS_NS;

ComputeCoordAtomMDP::ComputeCoordAtomMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "coord/atom/mdp", "there is no atom to count around"), cutoff(0.0)
{
  const std::string usage = "compute ID GROUP coord/atom/mdp cutoff Rc [jtype ...]";
  if (narg >= 4 && std::string(arg[3]) == "orientorder")
    error->all(FLERR, head + "the orientorder form is not supported: it counts the neighbours whose compute orientorder/atom vectors agree, "
                             "and there is none on the device; " + usage);
  if (narg < 5 || std::string(arg[3]) != "cutoff") error->all(FLERR, head + usage);
  cutoff = mdp_number(error, head, "Rc", arg[4], true);
  if (!(cutoff > 0.0)) error->all(FLERR, head + "Rc must be > 0, not " + arg[4]);
  const int ntypes = atom->ntypes;
  for (int iarg = 5; iarg < narg; iarg++) {
    if (std::string(arg[iarg]) == "group")
      error->all(FLERR, head + "the group keyword is not supported: the partners of a centre are the atoms of every group");
    int lo = 0, hi = 0;
    if (!mdp_type_bounds(arg[iarg], ntypes, lo, hi))
      error->all(FLERR, head + "type " + arg[iarg] + " is not N, *, N*, *M or N*M within 1 .. " + std::to_string(ntypes));
    jlo.push_back(lo);
    jhi.push_back(hi);
  }
  if (jlo.empty()) {
    jlo.push_back(1);
    jhi.push_back(ntypes);
  }
  if ((int) jlo.size() > MDP_COORD_MAXCOL)
    error->all(FLERR, head + std::to_string(jlo.size()) + " columns; at most " + std::to_string(MDP_COORD_MAXCOL) + " fit one compute");
  if (atom->natoms < 1) error->all(FLERR, "Compute coord/atom/mdp: there are no atoms");
  if (!atom->tag_enable) error->all(FLERR, "Compute coord/atom/mdp requires atom IDs");
  peratom_columns((int) jlo.size());
}

ComputeCoordAtomMDP::~ComputeCoordAtomMDP() {}

void ComputeCoordAtomMDP::init()
{
  require_bricks("where the host's atom->x and neighbour list are current: use compute coord/atom (or run the fix with bricks yes)");
  if (!force->pair) error->all(FLERR, "Compute coord/atom/mdp requires a pair style: its cutforce sets the ghost shell the partners come from");
  const double cutforce = force->pair->cutforce;
  if (cutoff > cutforce * (1.0 + 1e-12)) {
    char buf[320];
    snprintf(buf, sizeof buf, "Compute coord/atom/mdp: the cutoff %g is beyond the pair style's cutforce %.15g: the brick's ghost shell is cutforce + "
                              "skin wide as of the last reneighbouring, so only partners within cutforce are all present",
             cutoff, cutforce);
    error->all(FLERR, buf);
  }
  forget(); // a new run may bring a new context: the setup goes up again
}

void ComputeCoordAtomMDP::compute_peratom()
{
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_coord_info)) {
    if (mdp_coord_setup(c, cutoff, (int) jlo.size(), jlo.data(), jhi.data(), gbit()) != MDP_OK) fail(c);
    record(c, mdp_coord_info);
  }
  read_peratom(c, mdp_coord_read);
}
