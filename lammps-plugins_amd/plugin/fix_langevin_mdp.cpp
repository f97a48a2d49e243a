/* ------------------------------------------------------------------------------------------------
   fix langevin/mdp -- see fix_langevin_mdp.h.  What runs where:
     constructor        the arguments (refused here: an unknown or empty group, a group with atoms outside the integrator's
                        if that is defined already, variables, gjf / angmom / omega, bad numbers)
     init()             the one fix nve/mdp found through modify; a copy of the settings (with natoms, boltz, mvv2e)
                        written into this fix's slot of its Fix::extract("mdp_langevin_baths") block (mdp_riders.h) -- virtual
                        dispatch, since fix nve/mdp is compiled into several plugin files.  The slot is the fix's position
                        among the langevin/mdp fixes of Modify's list; refused here: a fifth langevin/mdp, and atoms in
                        the groups of two of them
     the steps          fix nve/mdp's: its setup() switches the thermostat on (mdp_langevin_setup / _run over
                        beginstep .. endstep) in the context the steps run on, its post_run() switches it off
     compute_scalar()   the tally of this fix's bath, read from the context of the run under way
   What it shares with the other fixes that ride on fix nve/mdp is FixRiderMDP's (fix_rider_mdp.h).
-------------------------------------------------------------------------------------------------- */
#include "fix_langevin_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "force.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace LAMMPS_NS;

namespace {
double number(LAMMPS *lmp, const char *s, const char *what)
{
  if (strncmp(s, "v_", 2) == 0)
    lmp->error->all(FLERR, std::string("Fix langevin/mdp: variables are not supported (") + what + " " + s + ")");
  return mdp_number(lmp->error, "Illegal fix langevin/mdp command: ", what, s);
}
} // namespace

FixLangevinMDP::FixLangevinMDP(LAMMPS *lmp, int narg, char **arg)
    : FixRiderMDP(lmp, narg, arg, "langevin/mdp", MDP_LANGEVIN_MAXBATH, "mdp_langevin_baths", 7,
                  "Illegal fix langevin/mdp command: fix ID all langevin/mdp Tstart Tstop damp seed [keywords]", "there is no atom to thermostat")
{
  memset(&cfg, 0, sizeof cfg);
  for (int t = 0; t < 16; t++) cfg.ratio[t] = 1.0;
  cfg.t_start = number(lmp, arg[3], "Tstart");
  cfg.t_stop = number(lmp, arg[4], "Tstop");
  cfg.t_period = number(lmp, arg[5], "damp");
  const double seed = number(lmp, arg[6], "seed");
  if (!(cfg.t_start >= 0.0) || !(cfg.t_stop >= 0.0)) error->all(FLERR, "Fix langevin/mdp: Tstart and Tstop must be >= 0.0");
  if (!(cfg.t_period > 0.0)) error->all(FLERR, "Fix langevin/mdp: damp must be > 0.0");
  if (!(seed >= 1.0) || seed > 2147483647.0 || seed != (double) (int) seed)
    error->all(FLERR, "Fix langevin/mdp: the seed must be an integer > 0");
  cfg.seed = (int) seed;
  for (int k = 7; k < narg;) {
    const std::string key = arg[k];
    if (key == "gjf" || key == "angmom" || key == "omega")
      error->all(FLERR, "Fix langevin/mdp: keyword " + key + " is not supported");
    if (key == "scale") {
      if (k + 2 >= narg) error->all(FLERR, "Illegal fix langevin/mdp command: scale needs a type and a ratio");
      const double t = number(lmp, arg[k + 1], "scale type");
      if (t < 1.0 || t > 15.0 || t != (double) (int) t || (atom && (int) t > atom->ntypes))
        error->all(FLERR, std::string("Fix langevin/mdp: scale type ") + arg[k + 1] + " out of range");
      const double r = number(lmp, arg[k + 2], "scale ratio");
      if (!(r > 0.0)) error->all(FLERR, "Fix langevin/mdp: the scale ratio must be > 0.0");
      cfg.ratio[(int) t] = r;
      k += 3;
      continue;
    }
    if (k + 1 >= narg) error->all(FLERR, "Illegal fix langevin/mdp command: " + key + " needs a value");
    if (key == "tally") cfg.tally = mdp_yesno(error, "Illegal fix langevin/mdp command: ", key, arg[k + 1], true);
    else if (key == "zero") cfg.zero = mdp_yesno(error, "Illegal fix langevin/mdp command: ", key, arg[k + 1], true);
    else error->all(FLERR, "Illegal fix langevin/mdp command: unknown keyword " + key);
    k += 2;
  }
  ecouple_flag = cfg.tally ? 1 : 0;
  if (Fix *nve = integrator()) inside(nve, "thermostat"); // (said here already when the integrator is defined; init() looks again)
  census(); // ... and so are a fifth bath and atoms shared with a bath defined before this one
  disjoint(); // (LAMMPS would add the forces of two thermostats on an atom that is in both groups)
}

void FixLangevinMDP::init()
{
  if ((cfg.zero || cfg.tally) && comm->nprocs > 1)
    error->all(FLERR, "Fix langevin/mdp: zero yes and tally yes run on one MPI rank only");
  int nbath = 0;
  Fix *nve = walk({"nvt/mdp"}, "", ") is a thermostat too; use one thermostat", "the device thermostat needs fix nve/mdp as the time integrator",
                  "Fix langevin/mdp requires fix nve/mdp as the time integrator", nbath);
  MdpLangevinBaths *block = static_cast<MdpLangevinBaths *>(handover(nve, "a thermostat"));
  inside(nve, "thermostat"); // (the thermostat acts inside the device's integrate pass)
  disjoint();
  // the atoms the thermostat acts on: its group, which lies inside the integrator's (zero yes divides by their number)
  cfg.boltz = force->boltz;
  cfg.mvv2e = force->mvv2e;
  cfg.natoms = (long long) populated();
  block->count = nbath;
  block->cfg[slot] = cfg;
  // one thermostat on the integrator's own group: bit 0, every atom the integrator moves (next to another bath that
  // group shares atoms with it and was refused above)
  block->bit[slot] = (nbath == 1 && igroup == nve->igroup) ? 0 : groupbit;
}

// FixLangevin::compute_scalar with tally yes: the energy the thermostat took out, back to the last full step
double FixLangevinMDP::compute_scalar()
{
  double e = 0.0;
  return cfg.tally && read(mdp_langevin_tally_bath, &e) ? e : 0.0;
}
