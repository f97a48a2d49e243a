/* ------------------------------------------------------------------------------------------------
   fix nvt/mdp -- see fix_nvt_mdp.h.  The steps are fix nve/mdp's (fix_nve_mdp.cpp) in its one-rank modes; what this
   subclass adds is the thermostat of the context those steps run on:
     setup()            mdp_nhc_setup with Tstart Tstop Tdamp tchain tloop drag, 3N - 3 degrees of freedom (N: the atoms of
                        the fix's group, whose temperature the chain sees and whose velocities it scales), force->boltz /
                        mvv2e; the chain of the previous run seeded again (mdp_nhc_set_state); the ramp of this run
                        (mdp_nhc_run, update->beginstep .. endstep)
     initial / final    fix nve/mdp's calls, which apply the chain on the device (mdp_hnve_*, mdp_md_integrate_check and
                        the pair style's final half-kick in `bricks yes` mode)
     post_run()         the chain read back (mdp_nhc_state) and the thermostat switched off on that context
     compute_scalar()   the thermostat energy (FixNH::compute_scalar) at the current target
-------------------------------------------------------------------------------------------------- */
#include "fix_nvt_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "force.h"
#include "update.h"
#ifndef MINILMP_LAMMPS_HOST_API_H
#include "modify.h"
#endif

#include <cstdlib>
#include <cstring>
#include <string>

using namespace LAMMPS_NS;

FixNVTMDP::Args FixNVTMDP::parse(LAMMPS *lmp, int narg, char **arg)
{
  Args a;
  memset(&a.cfg, 0, sizeof a.cfg);
  a.cfg.tchain = 3;
  a.cfg.tloop = 1;
  if (narg < 3) lmp->error->all(FLERR, "Illegal fix nvt/mdp command");
  for (int k = 0; k < 3; k++) a.nve.push_back(arg[k]);
  static const char *const barostat[] = {"iso", "aniso", "tri", "x", "y", "z", "xy", "xz", "yz", "couple", "ptemp", "mtk",
                                         "dilate", "pchain", "ploop", "nreset", "scalexy", "scalexz", "scaleyz", "flip",
                                         "fixedpoint", "update", "disc", "ext"};
  bool have_temp = false;
  for (int k = 3; k < narg;) {
    const std::string key = arg[k];
    for (const char *b : barostat)
      if (key == b) lmp->error->all(FLERR, "Fix nvt/mdp is a thermostat only: barostat keyword " + key + " is not supported");
    if (key == "temp") {
      if (k + 3 >= narg) lmp->error->all(FLERR, "Illegal fix nvt/mdp command: temp needs Tstart Tstop Tdamp");
      a.cfg.t_start = mdp_number(lmp->error, "Illegal fix nvt/mdp command: ", "Tstart", arg[k + 1]);
      a.cfg.t_stop = mdp_number(lmp->error, "Illegal fix nvt/mdp command: ", "Tstop", arg[k + 2]);
      a.cfg.t_period = mdp_number(lmp->error, "Illegal fix nvt/mdp command: ", "Tdamp", arg[k + 3]);
      have_temp = true;
      k += 4;
      continue;
    }
    if (k + 1 >= narg) lmp->error->all(FLERR, "Illegal fix nvt/mdp command: " + key + " needs a value");
    if (key == "tchain") a.cfg.tchain = atoi(arg[k + 1]);
    else if (key == "tloop") a.cfg.tloop = atoi(arg[k + 1]);
    else if (key == "drag") a.cfg.drag = mdp_number(lmp->error, "Illegal fix nvt/mdp command: ", "drag", arg[k + 1]);
    else if (key == "hostcheck" || key == "bricks") {
      a.nve.push_back(arg[k]);
      a.nve.push_back(arg[k + 1]);
    } else
      lmp->error->all(FLERR, "Illegal fix nvt/mdp command: unknown keyword " + key);
    k += 2;
  }
  if (!have_temp) lmp->error->all(FLERR, "Fix nvt/mdp requires the temp keyword (temp Tstart Tstop Tdamp)");
  if (!(a.cfg.t_start > 0.0) || !(a.cfg.t_stop > 0.0)) lmp->error->all(FLERR, "Fix nvt/mdp: Tstart and Tstop must be > 0.0");
  if (!(a.cfg.t_period > 0.0)) lmp->error->all(FLERR, "Fix nvt/mdp: Tdamp must be > 0.0");
  if (a.cfg.tchain < 1) lmp->error->all(FLERR, "Fix nvt/mdp: tchain must be >= 1");
  if (a.cfg.tchain > MDP_NHC_MAXCHAIN) lmp->error->all(FLERR, "Fix nvt/mdp: tchain must be <= " + std::to_string(MDP_NHC_MAXCHAIN));
  if (a.cfg.tloop < 1) lmp->error->all(FLERR, "Fix nvt/mdp: tloop must be >= 1");
  if (a.cfg.drag < 0.0) lmp->error->all(FLERR, "Fix nvt/mdp: drag must be >= 0.0");
  return a;
}

FixNVTMDP::FixNVTMDP(LAMMPS *lmp, int narg, char **arg) : FixNVTMDP(lmp, parse(lmp, narg, arg)) {}

FixNVTMDP::FixNVTMDP(LAMMPS *lmp, Args a) :
    FixNVEMDP(lmp, (int) a.nve.size(), a.nve.data()), ncfg(a.cfg), have_chain(0), nhc_ctx(nullptr), run_first(0), run_last(0)
{
  memset(chain, 0, sizeof chain);
  ecouple_flag = 1;
}

void FixNVTMDP::nhc_fail(mdp_ctx *c) { error->one(FLERR, std::string("Fix nvt/mdp: ") + (c ? mdp_last_error(c) : "no device context")); }

void FixNVTMDP::init()
{
  if (comm->nprocs != 1)
    error->all(FLERR, "Fix nvt/mdp runs on one MPI rank only: multi-rank NVT is not supported");
#ifndef MINILMP_LAMMPS_HOST_API_H
  for (int i = 0; i < modify->nfix; i++)
    if (modify->fix[i] != this && modify->fix[i]->time_integrate)
      error->all(FLERR, std::string("Fix nvt/mdp: fix ") + modify->fix[i]->id + " also integrates the atoms; use one time-integration fix");
#endif
  FixNVEMDP::init();
}

void FixNVTMDP::setup(int vflag)
{
  FixNVEMDP::setup(vflag);
  mdp_ctx *c = bricks ? bctx : ctx();
  if (!c) nhc_fail(nullptr);
  ncfg.nf = 3.0 * group_count() - 3.0; // (FixNH: the degrees of freedom of the fix's group)
  ncfg.boltz = force->boltz;
  ncfg.mvv2e = force->mvv2e;
  if (mdp_nhc_setup(c, &ncfg) != MDP_OK) nhc_fail(c);
  if (have_chain && mdp_nhc_set_state(c, chain) != MDP_OK) nhc_fail(c);
  run_first = update->beginstep;
  run_last = update->endstep;
  if (mdp_nhc_run(c, (long long) run_first, (long long) run_last) != MDP_OK) nhc_fail(c);
  nhc_ctx = c;
}

void FixNVTMDP::post_run()
{
  if (nhc_ctx) {
    if (mdp_nhc_state(nhc_ctx, chain) != MDP_OK) nhc_fail(nhc_ctx);
    have_chain = 1;
    if (mdp_nhc_off(nhc_ctx) != MDP_OK) nhc_fail(nhc_ctx); // (the pair style's context may serve another fix next)
    nhc_ctx = nullptr;
  }
  FixNVEMDP::post_run();
}

// FixNH::compute_scalar: the chain's energy at the target of the current step
double FixNVTMDP::compute_scalar()
{
  double st[MDP_NHC_STATE_LEN];
  if (nhc_ctx) {
    if (mdp_nhc_state(nhc_ctx, st) != MDP_OK) nhc_fail(nhc_ctx);
  } else
    memcpy(st, chain, sizeof st);
  const bigint n = update->ntimestep;
  const double delta = run_last == run_first ? 0.0 : (double) (n - run_first) / (double) (run_last - run_first);
  const double tt = ncfg.t_start + delta * (ncfg.t_stop - ncfg.t_start);
  const double kt = force->boltz * tt, tf = 1.0 / ncfg.t_period;
  const double nf = 3.0 * group_count() - 3.0;
  const double *eta = st + 3, *ed = st + 11;
  double q = nf * kt / (tf * tf);
  double e = nf * kt * eta[0] + 0.5 * q * ed[0] * ed[0];
  q = kt / (tf * tf);
  for (int i = 1; i < ncfg.tchain; i++) e += kt * eta[i] + 0.5 * q * ed[i] * ed[i];
  return e;
}
