/* ------------------------------------------------------------------------------------------------
   fix langevin/mdp -- see fix_langevin_mdp.h.  What runs where:
     constructor        the arguments (refused here: an unknown or empty group, a group with atoms outside the integrator's
                        if that is defined already, variables, gjf / angmom / omega, bad numbers)
     init()             the one fix nve/mdp found through modify; a copy of the settings (with natoms, boltz, mvv2e)
                        written into this fix's slot of its Fix::extract("mdp_langevin_baths") block (mdp_baths.h) -- virtual
                        dispatch, since fix nve/mdp is compiled into several plugin files.  The slot is the fix's position
                        among the langevin/mdp fixes of Modify's list; refused here: a fifth langevin/mdp, and atoms in
                        the groups of two of them
     the steps          fix nve/mdp's: its setup() switches the thermostat on (mdp_langevin_setup / _run over
                        beginstep .. endstep) in the context the steps run on, its post_run() switches it off
     compute_scalar()   the tally of this fix's bath, read through the context fix nve/mdp exposes (Fix::extract("mdp_run_ctx"))
-------------------------------------------------------------------------------------------------- */
#include "fix_langevin_mdp.h"
#include "mdp_args.h"
#include "mdp_baths.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "force.h"
#include "group.h"
#include "modify.h"

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

FixLangevinMDP::FixLangevinMDP(LAMMPS *lmp, int narg, char **arg) : Fix(lmp, narg, arg)
{
  memset(&cfg, 0, sizeof cfg);
  for (int t = 0; t < 16; t++) cfg.ratio[t] = 1.0;
  if (narg < 7) error->all(FLERR, "Illegal fix langevin/mdp command: fix ID all langevin/mdp Tstart Tstop damp seed [keywords]");
  if (igroup < 0)
    error->all(FLERR, std::string("Fix langevin/mdp requires group all or a group defined by the group command: could not find fix group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Fix langevin/mdp: group ") + arg[1] + " is empty: there is no atom to thermostat");
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
  if (Fix *nve = integrator()) inside(nve); // (said here already when the integrator is defined; init() looks again)
  int earlier = 0; // ... and so are a fifth bath and atoms shared with a bath defined before this one
  for (int i = 0; i < modify->nfix; i++)
    if (strcmp(modify->fix[i]->style, "langevin/mdp") == 0) earlier++;
  if (earlier + 1 > MDP_LANGEVIN_MAXBATH) too_many(earlier + 1);
  disjoint();
}

void FixLangevinMDP::too_many(int n)
{
  error->all(FLERR, std::string("Fix langevin/mdp: ") + id + " is langevin/mdp fix number " + std::to_string(n) + "; fix nve/mdp takes up to " +
                        std::to_string(MDP_LANGEVIN_MAXBATH) + " of them");
}

// Several baths: LAMMPS would add the forces of two thermostats on an atom that is in both groups; the device's one pass
// gives an atom one bath, so shared atoms are refused.  Every langevin/mdp fix before this one in Modify's list is looked
// at (all of them while this fix is being constructed: it is not in the list yet), so each pair is looked at once.
void FixLangevinMDP::disjoint()
{
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (f == this) break;
    if (strcmp(f->style, "langevin/mdp") != 0) continue;
    double mine = 0.0, shared = 0.0;
    for (int a = 0; a < atom->nlocal; a++)
      if ((atom->mask[a] & groupbit) && (atom->mask[a] & f->groupbit)) mine += 1.0;
    MPI_Allreduce(&mine, &shared, 1, MPI_DOUBLE, MPI_SUM, world);
    if (shared > 0.0)
      error->all(FLERR, std::string("Fix langevin/mdp: fixes ") + f->id + " and " + id + " share " + std::to_string((long long) shared) +
                            " atoms (groups " + group->names[f->igroup] + " and " + group->names[igroup] +
                            "); the groups of several langevin/mdp fixes must be disjoint");
  }
}

// the thermostat acts inside the device's integrate pass: an atom it is to thermostat must be one the integrator moves
void FixLangevinMDP::inside(Fix *nve)
{
  if (igroup == nve->igroup || nve->igroup == 0) return;
  long outside = 0;
  for (int i = 0; i < atom->nlocal; i++)
    if ((atom->mask[i] & groupbit) && !(atom->mask[i] & nve->groupbit)) outside++;
  if (outside)
    error->one(FLERR, std::string("Fix langevin/mdp: group ") + group->names[igroup] + " has " + std::to_string(outside) +
                          " atoms outside group " + group->names[nve->igroup] + " of fix " + nve->id +
                          " (nve/mdp): the thermostat acts on atoms the integrator moves");
}

int FixLangevinMDP::setmask() { return 0; } // (the force is applied inside fix nve/mdp's device steps)

Fix *FixLangevinMDP::integrator() const
{
  for (int i = 0; i < modify->nfix; i++)
    if (strcmp(modify->fix[i]->style, "nve/mdp") == 0) return modify->fix[i];
  return nullptr;
}

void FixLangevinMDP::init()
{
  if ((cfg.zero || cfg.tally) && comm->nprocs > 1)
    error->all(FLERR, "Fix langevin/mdp: zero yes and tally yes run on one MPI rank only");
  Fix *nve = nullptr;
  int nbath = 0;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "langevin/mdp") == 0) { // (this fix among them: its slot is its position in the list)
      if (f == this) bath = nbath;
      nbath++;
      continue;
    }
    if (strcmp(f->style, "nvt/mdp") == 0)
      error->all(FLERR, std::string("Fix langevin/mdp: fix ") + f->id + " (nvt/mdp) is a thermostat too; use one thermostat");
    if (strcmp(f->style, "nve/mdp") == 0) nve = f;
    else if (f->time_integrate)
      error->all(FLERR, std::string("Fix langevin/mdp: fix ") + f->id + " (" + f->style +
                            ") integrates on the host; the device thermostat needs fix nve/mdp as the time integrator");
  }
  if (!nve) error->all(FLERR, "Fix langevin/mdp requires fix nve/mdp as the time integrator");
  if (nbath > MDP_LANGEVIN_MAXBATH) too_many(nbath);
  int dim = 0;
  MdpLangevinBaths *block = static_cast<MdpLangevinBaths *>(nve->extract("mdp_langevin_baths", dim));
  if (!block) error->all(FLERR, "Fix langevin/mdp: this fix nve/mdp does not take a thermostat");
  inside(nve);
  disjoint(); // (several baths: no atom in two of them)
  // the atoms the thermostat acts on: its group, which lies inside the integrator's (zero yes divides by their number)
  const int acts = igroup;
  cfg.boltz = force->boltz;
  cfg.mvv2e = force->mvv2e;
  cfg.natoms = acts == 0 ? (long long) atom->natoms : (long long) group->count(acts);
  if (cfg.natoms < 1) error->all(FLERR, std::string("Fix langevin/mdp: group ") + group->names[acts] + " is empty: there is no atom to thermostat");
  block->count = nbath;
  block->cfg[bath] = cfg;
  // one thermostat on the integrator's own group: bit 0, every atom the integrator moves (next to another bath that
  // group shares atoms with it and was refused above)
  block->bit[bath] = (nbath == 1 && igroup == nve->igroup) ? 0 : groupbit;
}

// FixLangevin::compute_scalar with tally yes: the energy the thermostat took out, back to the last full step
double FixLangevinMDP::compute_scalar()
{
  if (!cfg.tally) return 0.0;
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **c = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_run_ctx", dim)) : nullptr;
  if (!c || !*c) return 0.0;
  double e = 0.0;
  if (mdp_langevin_tally_bath(*c, bath, &e) != MDP_OK) error->one(FLERR, std::string("Fix langevin/mdp: ") + mdp_last_error(*c));
  return e;
}
