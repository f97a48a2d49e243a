/* ------------------------------------------------------------------------------------------------
   minimize/mdp -- see command_minimize_mdp.h
-------------------------------------------------------------------------------------------------- */
#include "command_minimize_mdp.h"
#include "mdp_args.h"
#include "mdp_brick.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "group.h"
#include "modify.h"
#include "neighbor.h"
#include "output.h"
#include "pair.h"
#include "update.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace LAMMPS_NS;

namespace {

const char *kCriterion[] = {"running", "force tolerance", "energy tolerance", "max iterations", "max force evaluations"};

} // namespace

MinimizeMDP::~MinimizeMDP()
{
  if (ctx) mdp_destroy(ctx);
}

void MinimizeMDP::fail(const char *what)
{
  error->one(FLERR, std::string("minimize/mdp: ") + what + ": " + (ctx ? mdp_last_error(ctx) : "no device context"));
}

// the arguments alone: everything here is refused before a device is touched
void MinimizeMDP::parse(int narg, char **arg)
{
  if (narg < 4) error->all(FLERR, "Illegal minimize/mdp command: expected etol ftol maxiter maxeval");
  memset(&cfg, 0, sizeof cfg);
  if (!mdp_number(arg[0], cfg.etol, true) || !mdp_number(arg[1], cfg.ftol, true))
    error->all(FLERR, "minimize/mdp: etol and ftol must be numbers");
  if (!mdp_whole(arg[2], cfg.maxiter) || !mdp_whole(arg[3], cfg.maxeval))
    error->all(FLERR, "minimize/mdp: maxiter and maxeval must be integers");
  if (cfg.etol < 0.0 || cfg.ftol < 0.0) error->all(FLERR, "minimize/mdp: etol and ftol must be >= 0.0");
  if (cfg.maxiter < 0 || cfg.maxeval < 0) error->all(FLERR, "minimize/mdp: maxiter and maxeval must be >= 0");
  // LAMMPS' min_modify defaults for min_style fire
  cfg.dmax = 0.1;
  cfg.tmax = 10.0;
  cfg.tmin = 0.02;
  cfg.delaystep = 20;
  cfg.dtgrow = 1.1;
  cfg.dtshrink = 0.5;
  cfg.alpha0 = 0.25;
  cfg.alphashrink = 0.99;
  cfg.halfstepback = 1;
  cfg.initialdelay = 1;
  igroup = 0;
  for (int k = 4; k < narg; k += 2) {
    const std::string key = arg[k];
    if (key == "group") { // the atoms that move; the others are held (fix setforce 0 0 0 on them)
      if (k + 1 >= narg) error->all(FLERR, "minimize/mdp: group needs a group ID");
      igroup = group->find(arg[k + 1]);
      if (igroup < 0) error->all(FLERR, std::string("minimize/mdp: could not find group ID ") + arg[k + 1]);
      if (igroup > 0 && group->count(igroup) == 0)
        error->all(FLERR, std::string("minimize/mdp: group ") + arg[k + 1] + " is empty: there is no atom to move");
      continue;
    }
    if (key == "integrator" || key == "norm" || key == "line")
      error->all(FLERR, "minimize/mdp: keyword " + key + " is not supported (integrator eulerimplicit, norm two, no line search)");
    const bool known = key == "dmax" || key == "tmax" || key == "tmin" || key == "delaystep" || key == "dtgrow" ||
        key == "dtshrink" || key == "alpha0" || key == "alphashrink" || key == "halfstepback" || key == "initialdelay";
    if (!known) error->all(FLERR, "minimize/mdp: unknown keyword " + key);
    if (k + 1 >= narg) error->all(FLERR, "minimize/mdp: " + key + " needs a value");
    const std::string val = arg[k + 1];
    if (key == "halfstepback" || key == "initialdelay") {
      (key == "halfstepback" ? cfg.halfstepback : cfg.initialdelay) = mdp_yesno(error, "minimize/mdp: ", key, val.c_str(), false);
      continue;
    }
    long long n = 0;
    if (key == "delaystep") {
      if (!mdp_whole(val.c_str(), n) || n < 0 || n > 1000000000) error->all(FLERR, "minimize/mdp: delaystep must be an integer >= 0");
      cfg.delaystep = (int) n;
      continue;
    }
    const double v = mdp_number(error, "minimize/mdp: ", key, val.c_str(), true);
    if (key == "dmax") {
      if (v <= 0.0) error->all(FLERR, "minimize/mdp: dmax must be > 0.0");
      cfg.dmax = v;
    } else if (key == "tmax") {
      if (v < 1.0) error->all(FLERR, "minimize/mdp: tmax must be >= 1.0");
      cfg.tmax = v;
    } else if (key == "tmin") {
      if (v <= 0.0 || v > 1.0) error->all(FLERR, "minimize/mdp: tmin must be > 0.0 and <= 1.0");
      cfg.tmin = v;
    } else if (key == "dtgrow") {
      if (v < 1.0) error->all(FLERR, "minimize/mdp: dtgrow must be >= 1.0");
      cfg.dtgrow = v;
    } else if (key == "dtshrink") {
      if (v <= 0.0 || v > 1.0) error->all(FLERR, "minimize/mdp: dtshrink must be > 0.0 and <= 1.0");
      cfg.dtshrink = v;
    } else if (key == "alpha0") {
      if (v <= 0.0 || v >= 1.0) error->all(FLERR, "minimize/mdp: alpha0 must be > 0.0 and < 1.0");
      cfg.alpha0 = v;
    } else { // alphashrink
      if (v <= 0.0 || v > 1.0) error->all(FLERR, "minimize/mdp: alphashrink must be > 0.0 and <= 1.0");
      cfg.alphashrink = v;
    }
  }
}

void MinimizeMDP::command(int narg, char **arg)
{
  parse(narg, arg);
  if (comm->nprocs != 1)
    error->all(FLERR, "minimize/mdp runs on one MPI rank (its sums would need an all-reduce per iteration)");
  if (!domain->xperiodic || !domain->yperiodic || !domain->zperiodic) error->all(FLERR, "minimize/mdp needs a periodic box");
  for (int i = 0; i < modify->nfix; i++) // (LAMMPS' minimiser would add the indenters' forces; this one sees the pair style's alone)
    if (strcmp(modify->fix[i]->style, "indent/mdp") == 0)
      error->all(FLERR, std::string("minimize/mdp: fix ") + modify->fix[i]->id + " (indent/mdp) is not applied by the minimiser; unfix it first");
    else if (strcmp(modify->fix[i]->style, "spring/mdp") == 0)
      error->all(FLERR, std::string("minimize/mdp: fix ") + modify->fix[i]->id + " (spring/mdp) is not applied by the minimiser; unfix it first");
    else if (strcmp(modify->fix[i]->style, "setforce/mdp") == 0 || strcmp(modify->fix[i]->style, "addforce/mdp") == 0 ||
             strcmp(modify->fix[i]->style, "aveforce/mdp") == 0)
      error->all(FLERR, std::string("minimize/mdp: fix ") + modify->fix[i]->id + " (" + modify->fix[i]->style +
                            ") is not applied by the minimiser; unfix it first");
  const int style_id = mdp_pair_style_id(force->pair);
  if (!style_id) error->all(FLERR, "minimize/mdp requires a pair style of this plugin (rebomos or aeam)");
  if (const char *e = getenv("MDP_REBOMOS_HOST_LIST"))
    if (style_id == 1 && atoi(e) != 0)
      error->all(FLERR, "minimize/mdp keeps the atoms on the device and cannot be combined with MDP_REBOMOS_HOST_LIST=1");
  if (!(update->dt > 0.0)) error->all(FLERR, "minimize/mdp: the timestep must be > 0.0");

  const mdp_own_context_result own = mdp_own_context(force->pair, comm->me, &ctx);
  if (own.why) error->all(FLERR, std::string("minimize/mdp") + own.why);
  if (own.failed && !ctx) error->one(FLERR, "minimize/mdp needs a HIP device: cannot create a device context");
  if (own.failed) fail(own.failed);
  const bool with_mask = igroup > 0 || mdp_host_has_groups(group);
  if (mdp_brick_from_host(ctx, style_id, own.map, atom, domain, force, neighbor, update, comm, with_mask) != MDP_OK) fail("setup");
  if (mdp_dd_reneighbor(ctx) != MDP_OK) fail("lists");
  if (mdp_integrate_group(ctx, igroup > 0 ? group->bitmask[igroup] : 0) != MDP_OK) fail("group");
  if (mdp_fire_setup(ctx, &cfg) != MDP_OK) fail("setup");

  const bigint step0 = update->ntimestep;
  const long long every = output->thermo_every > 0 ? output->thermo_every : 0;
  double st[MDP_FIRE_STATE_LEN];
  auto row = [&]() { // (a blocking read; with etol == 0 also one energy compute)
    if (mdp_fire_state(ctx, st) != MDP_OK) fail("state");
    if (comm->me == 0) printf("%10lld %18.12g %18.12g\n", (long long) step0 + (long long) st[1], st[8], st[5]);
  };
  if (every && comm->me == 0) printf("      Step          PotEng              Fnorm\n");
  if (every) row();
  // (the stop code is seen an iteration or two late: what was queued too many changes nothing)
  int stop = 0;
  long long left = cfg.maxiter + 2;
  while (!stop && left > 0) {
    const long long n = every ? (every < left ? every : left) : (left < 256 ? left : 256);
    if (mdp_fire_iterate(ctx, n, &stop) != MDP_OK) fail("iteration");
    left -= n;
    if (every && !stop && left > 0) row();
  }
  if (mdp_fire_state(ctx, st) != MDP_OK) fail("state");
  if (every && comm->me == 0) printf("%10lld %18.12g %18.12g\n", (long long) step0 + (long long) st[1], st[8], st[5]);
  if (mdp_fire_off(ctx) != MDP_OK) fail("off");
  if (mdp_brick_to_host(ctx, atom, with_mask) != MDP_OK) fail("return of the atoms");
  update->ntimestep = step0 + (bigint) st[1];
  const int code = (int) st[0];
  if (comm->me == 0) {
    printf("Minimization stats:\n");
    printf("  Stopping criterion = %s\n", kCriterion[code >= 0 && code <= 4 ? code : 0]);
    printf("  Energy initial, next-to-last, final = \n    %18.12g %18.12g %18.12g\n", st[6], st[7], st[8]);
    printf("  Force two-norm initial, final = %.8g %.8g\n", st[19], st[5]);
    printf("  Iterations, force evaluations = %lld %lld\n", (long long) st[1], (long long) st[2]);
    printf("  Reneighborings on the device = %lld\n", (long long) st[9]);
  }
  mdp_destroy(ctx);
  ctx = nullptr;
}
