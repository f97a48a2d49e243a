/* ------------------------------------------------------------------------------------------------
   compute centro/atom/mdp -- see compute_centro_atom_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: no lattice word, an N that is no whole number,
                        odd, below 2 or above 64, the axes keyword, an unknown keyword, a bad or non-positive Rc)
     init()             bricks mode (the host-linked mode: there the host's atom->x and neighbour list are current, and compute
                        centro/atom is right); Rc against the pair style's cutforce, which is also its default
     compute_peratom()  the setup goes up once per context and run (mdp_centro_setup); mdp_centro_read on this rank's brick, into
                        vector_atom behind the check of the tags (compute_mdp.h, read_peratom).  A centre with more than 128
                        atoms inside Rc ends the run here with the library's message, which names cutoff.
   The group refusals, the integrator, the run's context and the once-per-context protocol: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_centro_atom_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "error.h"
#include "force.h"
#include "pair.h"

#include <string>

using namespace LAMMPS_NS;

ComputeCentroAtomMDP::ComputeCentroAtomMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "centro/atom/mdp", "there is no atom to look around"), nnn(0), cutoff(0.0)
{
  const std::string usage = "compute ID GROUP centro/atom/mdp fcc|bcc|N [cutoff Rc]";
  if (narg < 4) error->all(FLERR, head + usage);
  const std::string lat = arg[3];
  if (lat == "fcc") nnn = 12;
  else if (lat == "bcc") nnn = 8;
  else {
    long long n = 0;
    if (!mdp_whole(arg[3], n)) error->all(FLERR, head + "the lattice is fcc, bcc or a whole number N of neighbours, not " + lat);
    if (n < 2 || n % 2) error->all(FLERR, head + "N must be an even whole number >= 2, not " + lat);
    if (n > MDP_CENTRO_MAXN)
      error->all(FLERR, head + "N = " + lat + "; at most " + std::to_string(MDP_CENTRO_MAXN) + " neighbours fit the device's list of pair values");
    nnn = (int) n;
  }
  for (int iarg = 4; iarg < narg; iarg += 2) {
    const std::string key = arg[iarg];
    if (key == "axes")
      error->all(FLERR, head + "the axes keyword is not supported: the compute is a per-atom vector, the centro-symmetry parameter alone");
    if (key != "cutoff") error->all(FLERR, head + "unknown keyword " + key);
    if (iarg + 1 >= narg) error->all(FLERR, head + "cutoff needs a value");
    cutoff = mdp_number(error, head, "Rc", arg[iarg + 1], true);
    if (!(cutoff > 0.0)) error->all(FLERR, head + "Rc must be > 0, not " + arg[iarg + 1]);
  }
  if (atom->natoms < 1) error->all(FLERR, "Compute centro/atom/mdp: there are no atoms");
  if (!atom->tag_enable) error->all(FLERR, "Compute centro/atom/mdp requires atom IDs");
  peratom_columns(1);
}

ComputeCentroAtomMDP::~ComputeCentroAtomMDP() {}

void ComputeCentroAtomMDP::init()
{
  require_bricks("where the host's atom->x and neighbour list are current: use compute centro/atom (or run the fix with bricks yes)");
  if (!force->pair) error->all(FLERR, "Compute centro/atom/mdp requires a pair style: its cutforce sets the ghost shell the neighbours come from");
  const double cutforce = force->pair->cutforce;
  if (cutoff > cutforce * (1.0 + 1e-12)) {
    char buf[320];
    snprintf(buf, sizeof buf, "Compute centro/atom/mdp: the cutoff %g is beyond the pair style's cutforce %.15g: the brick's ghost shell is cutforce + "
                              "skin wide as of the last reneighbouring, so only neighbours within cutforce are all present",
             cutoff, cutforce);
    error->all(FLERR, buf);
  }
  forget(); // a new run may bring a new context: the setup goes up again
}

void ComputeCentroAtomMDP::compute_peratom()
{
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_centro_info)) {
    if (mdp_centro_setup(c, nnn, cutoff, gbit()) != MDP_OK) fail(c); // (cutoff 0: the shell's limit, cutghost - skin = cutforce)
    record(c, mdp_centro_info);
  }
  read_peratom(c, mdp_centro_read);
}
