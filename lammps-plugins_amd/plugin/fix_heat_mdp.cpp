/* ------------------------------------------------------------------------------------------------
   fix heat/mdp -- see fix_heat_mdp.h.  What runs where:
     constructor        the arguments (refused here, before a device is touched: an unknown or empty group, N < 1, a
                        variable as eflux, the region keyword, a fifth heat/mdp, atoms shared with an earlier heat/mdp,
                        atoms outside the integrator's group if that is defined already)
     init()             the one fix nve/mdp found through modify; a copy of the settings (with mvv2e) written into this
                        fix's slot of its Fix::extract("mdp_heat_sources") block (mdp_riders.h).  Refused here: no fix
                        nve/mdp, a host-side time integrator, a thermostat of this plugin in the same run, several ranks
     the steps          fix nve/mdp's: its setup() switches the sources on (mdp_heat_setup, mdp_heat_run(beginstep)) in the
                        context the steps run on, its post_run() switches them off
     compute_scalar()   the scale of this fix's last application, read from the context of the run under way
   What it shares with the other fixes that ride on fix nve/mdp is FixRiderMDP's (fix_rider_mdp.h).
-------------------------------------------------------------------------------------------------- */
#include "fix_heat_mdp.h"
#include "mdp_args.h"

#include "comm.h"
#include "error.h"
#include "force.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

FixHeatMDP::FixHeatMDP(LAMMPS *lmp, int narg, char **arg)
    : FixRiderMDP(lmp, narg, arg, "heat/mdp", MDP_HEAT_MAXSRC, "mdp_heat_sources", 5, "Illegal fix heat/mdp command: fix ID group heat/mdp N eflux",
                  "there is no atom to heat")
{
  memset(&cfg, 0, sizeof cfg);
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
  census();
  disjoint(); // (LAMMPS would rescale an atom in two groups twice)
  if (Fix *nve = integrator()) inside(nve, "source"); // (said here already when the integrator is defined; init() looks again)
}

void FixHeatMDP::init()
{
  if (comm->nprocs > 1) error->all(FLERR, "Fix heat/mdp runs on one MPI rank only (its sums are taken on one device)");
  int nsrc = 0;
  Fix *nve = walk({"nvt/mdp", "langevin/mdp"}, std::string(id) + " cannot run next to fix ", "): heat sources run without a thermostat; unfix one of them",
                  "the device's heat sources need fix nve/mdp as the time integrator", "Fix heat/mdp requires fix nve/mdp as the time integrator", nsrc);
  MdpHeatSources *block = static_cast<MdpHeatSources *>(handover(nve, "heat sources"));
  inside(nve, "source"); // (the sources rescale velocities behind the device's final half)
  disjoint();
  populated();
  cfg.mvv2e = force->mvv2e;
  block->count = nsrc;
  block->cfg[slot] = cfg;
  block->bit[slot] = groupbit;
}

// FixHeat::compute_scalar: the scale of the last application; between runs what the last read returned
double FixHeatMDP::compute_scalar()
{
  double st[MDP_HEAT_STATE_LEN];
  if (read(mdp_heat_state, st)) scale = st[0];
  return scale;
}
