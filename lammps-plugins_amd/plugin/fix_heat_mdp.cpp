/* ------------------------------------------------------------------------------------------------
   fix heat/mdp -- see fix_heat_mdp.h.  What runs where:
     constructor        the arguments (refused here, before a device is touched: an unknown or empty group, N < 1, a
                        variable as eflux, the region keyword, a fifth heat/mdp, atoms shared with an earlier heat/mdp,
                        atoms outside the integrator's group if that is defined already)
     init()             the one fix nve/mdp found through modify; a copy of the settings (with mvv2e) written into this
                        fix's slot of its Fix::extract("mdp_heat_sources") block (mdp_heat.h).  Refused here: no fix
                        nve/mdp, a host-side time integrator, a thermostat of this plugin in the same run, several ranks
     the steps          fix nve/mdp's: its setup() switches the sources on (mdp_heat_setup, mdp_heat_run(beginstep)) in the
                        context the steps run on, its post_run() switches them off
     compute_scalar()   the scale of this fix's last application, read through the context fix nve/mdp exposes
                        (Fix::extract("mdp_heat_ctx"))
-------------------------------------------------------------------------------------------------- */
#include "fix_heat_mdp.h"
#include "mdp_args.h"
#include "mdp_heat.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "force.h"
#include "group.h"
#include "modify.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

FixHeatMDP::FixHeatMDP(LAMMPS *lmp, int narg, char **arg) : Fix(lmp, narg, arg)
{
  memset(&cfg, 0, sizeof cfg);
  if (narg < 5) error->all(FLERR, "Illegal fix heat/mdp command: fix ID group heat/mdp N eflux");
  if (igroup < 0)
    error->all(FLERR, std::string("Fix heat/mdp requires group all or a group defined by the group command: could not find fix group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Fix heat/mdp: group ") + arg[1] + " is empty: there is no atom to heat");
  long long n = 0;
  if (!mdp_whole(arg[3], n)) error->all(FLERR, std::string("Illegal fix heat/mdp command: bad N value ") + arg[3]);
  if (n < 1 || n > 2147483647LL) error->all(FLERR, "Fix heat/mdp: N must be >= 1");
  cfg.nevery = (int) n;
  if (strncmp(arg[4], "v_", 2) == 0)
    error->all(FLERR, std::string("Fix heat/mdp: a variable as eflux is not supported (") + arg[4] + "); the flux is constant");
  cfg.eflux = mdp_number(error, "Illegal fix heat/mdp command: ", "eflux", arg[4], true);
  for (int k = 5; k < narg; k++) {
    if (strcmp(arg[k], "region") == 0) error->all(FLERR, "Fix heat/mdp: keyword region is not supported; the source is its group");
    error->all(FLERR, std::string("Illegal fix heat/mdp command: unknown keyword ") + arg[k]);
  }
#ifndef MINILMP_LAMMPS_HOST_API_H
  scalar_flag = 1; // (thermo f_ID under LAMMPS; the mini-host's Fix prints compute_scalar() without these)
  global_freq = cfg.nevery;
  extscalar = 0;
#endif
  int earlier = 0;
  for (int i = 0; i < modify->nfix; i++)
    if (strcmp(modify->fix[i]->style, "heat/mdp") == 0) earlier++;
  if (earlier + 1 > MDP_HEAT_MAXSRC) too_many(earlier + 1);
  disjoint();
  if (Fix *nve = integrator()) inside(nve); // (said here already when the integrator is defined; init() looks again)
}

void FixHeatMDP::too_many(int n)
{
  error->all(FLERR, std::string("Fix heat/mdp: ") + id + " is heat/mdp fix number " + std::to_string(n) + "; fix nve/mdp takes up to " +
                        std::to_string(MDP_HEAT_MAXSRC) + " of them");
}

// LAMMPS would rescale an atom in two groups twice; the device's one pass gives an atom one source, so shared atoms are
// refused.  Every heat/mdp fix before this one in Modify's list is looked at (all of them while this fix is being
// constructed: it is not in the list yet), so each pair is looked at once.
void FixHeatMDP::disjoint()
{
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (f == this) break;
    if (strcmp(f->style, "heat/mdp") != 0) continue;
    double mine = 0.0, shared = 0.0;
    for (int a = 0; a < atom->nlocal; a++)
      if ((atom->mask[a] & groupbit) && (atom->mask[a] & f->groupbit)) mine += 1.0;
    MPI_Allreduce(&mine, &shared, 1, MPI_DOUBLE, MPI_SUM, world);
    if (shared > 0.0)
      error->all(FLERR, std::string("Fix heat/mdp: fixes ") + f->id + " and " + id + " share " + std::to_string((long long) shared) +
                            " atoms (groups " + group->names[f->igroup] + " and " + group->names[igroup] +
                            "); the groups of several heat/mdp fixes must be disjoint");
  }
}

// the sources rescale velocities behind the device's final half: an atom they act on must be one the integrator moves
void FixHeatMDP::inside(Fix *nve)
{
  if (igroup == nve->igroup || nve->igroup == 0) return;
  long outside = 0;
  for (int i = 0; i < atom->nlocal; i++)
    if ((atom->mask[i] & groupbit) && !(atom->mask[i] & nve->groupbit)) outside++;
  if (outside)
    error->one(FLERR, std::string("Fix heat/mdp: group ") + group->names[igroup] + " has " + std::to_string(outside) +
                          " atoms outside group " + group->names[nve->igroup] + " of fix " + nve->id +
                          " (nve/mdp): the source acts on atoms the integrator moves");
}

int FixHeatMDP::setmask() { return 0; } // (the pass runs inside fix nve/mdp's device steps)

Fix *FixHeatMDP::integrator() const
{
  for (int i = 0; i < modify->nfix; i++)
    if (strcmp(modify->fix[i]->style, "nve/mdp") == 0) return modify->fix[i];
  return nullptr;
}

void FixHeatMDP::init()
{
  if (comm->nprocs > 1) error->all(FLERR, "Fix heat/mdp runs on one MPI rank only (its sums are taken on one device)");
  Fix *nve = nullptr;
  int nsrc = 0;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "heat/mdp") == 0) { // (this fix among them: its slot is its position in the list)
      if (f == this) src = nsrc;
      nsrc++;
      continue;
    }
    if (strcmp(f->style, "nvt/mdp") == 0 || strcmp(f->style, "langevin/mdp") == 0)
      error->all(FLERR, std::string("Fix heat/mdp: fix ") + id + " cannot run next to fix " + f->id + " (" + f->style +
                            "): heat sources run without a thermostat; unfix one of them");
    if (strcmp(f->style, "nve/mdp") == 0) nve = f;
    else if (f->time_integrate)
      error->all(FLERR, std::string("Fix heat/mdp: fix ") + f->id + " (" + f->style +
                            ") integrates on the host; the device's heat sources need fix nve/mdp as the time integrator");
  }
  if (!nve) error->all(FLERR, "Fix heat/mdp requires fix nve/mdp as the time integrator");
  if (nsrc > MDP_HEAT_MAXSRC) too_many(nsrc);
  int dim = 0;
  MdpHeatSources *block = static_cast<MdpHeatSources *>(nve->extract("mdp_heat_sources", dim));
  if (!block) error->all(FLERR, "Fix heat/mdp: this fix nve/mdp does not take heat sources");
  inside(nve);
  disjoint();
  if ((igroup == 0 ? (double) atom->natoms : (double) group->count(igroup)) < 1.0)
    error->all(FLERR, std::string("Fix heat/mdp: group ") + group->names[igroup] + " is empty: there is no atom to heat");
  cfg.mvv2e = force->mvv2e;
  block->count = nsrc;
  block->cfg[src] = cfg;
  block->bit[src] = groupbit;
}

// FixHeat::compute_scalar: the scale of the last application; between runs what the last read returned
double FixHeatMDP::compute_scalar()
{
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **c = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_heat_ctx", dim)) : nullptr;
  if (!c || !*c) return scale;
  double st[MDP_HEAT_STATE_LEN];
  if (mdp_heat_state(*c, src, st) != MDP_OK) error->one(FLERR, std::string("Fix heat/mdp: ") + mdp_last_error(*c));
  scale = st[0];
  return scale;
}
