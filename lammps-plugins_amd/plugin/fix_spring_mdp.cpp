/* ------------------------------------------------------------------------------------------------
   fix spring/mdp -- see fix_spring_mdp.h.  What runs where:
     constructor        the arguments (refused here, before a device is touched: an unknown or empty group, couple, a
                        variable anywhere, bad or negative K or R0, x, y and z all NULL, an unknown keyword, a fifth
                        spring/mdp)
     init()             the one fix nve/mdp found through modify; a copy of the settings written into this fix's slot of its
                        Fix::extract("mdp_springs") block (mdp_riders.h).  Refused here: no fix nve/mdp, one without bricks
                        yes, a host-side time integrator, fix nvt/mdp or fix heat/mdp in the same run, several ranks, atoms
                        of the group that the integrator does not move
     the steps          fix nve/mdp's: its setup() switches the springs on (mdp_spring_setup, mdp_spring_run(beginstep)),
                        behind the indenters, in the context the steps run on; its post_run() switches them off
     compute_scalar()   the spring's energy, compute_vector(0..3) ftotal, read from the context of the run under way, once
                        per step
   What it shares with the other fixes that ride on fix nve/mdp is FixRiderMDP's (fix_rider_mdp.h).
-------------------------------------------------------------------------------------------------- */
#include "fix_spring_mdp.h"
#include "mdp_args.h"

#include "comm.h"
#include "error.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

double FixSpringMDP::number(const char *what, const char *s)
{
  if (strncmp(s, "v_", 2) == 0)
    error->all(FLERR, std::string("Fix spring/mdp: a variable as ") + what + " is not supported (" + s + "); a moving tether point takes vel vx vy vz");
  return mdp_number(error, "Illegal fix spring/mdp command: ", what, s, true);
}

static const char *const usage = "Illegal fix spring/mdp command: fix ID group spring/mdp tether K x y z R0 [vel vx vy vz]";

FixSpringMDP::FixSpringMDP(LAMMPS *lmp, int narg, char **arg)
    : FixRiderMDP(lmp, narg, arg, "spring/mdp", MDP_SPRING_MAX, "mdp_springs", 4, usage, "there is no centre of mass to pull on")
{
  memset(&cfg, 0, sizeof cfg);
  if (strcmp(arg[3], "couple") == 0)
    error->all(FLERR, "Fix spring/mdp: couple is not supported; only tether is (a spring between a group and a point)");
  if (strcmp(arg[3], "tether") != 0) error->all(FLERR, std::string("Illegal fix spring/mdp command: unknown mode ") + arg[3] + " (tether)");
  for (int k = 4; k < narg; k++) // (a variable is named as such wherever it stands, before anything else is said)
    if (strncmp(arg[k], "v_", 2) == 0) number("an argument", arg[k]);
  if (narg < 9) error->all(FLERR, usage);
  cfg.k = number("K", arg[4]);
  if (cfg.k < 0.0) error->all(FLERR, "Fix spring/mdp: K must be >= 0.0");
  const char *names[3] = {"x", "y", "z"};
  for (int d = 0; d < 3; d++) {
    cfg.use[d] = strcmp(arg[5 + d], "NULL") != 0;
    cfg.c[d] = cfg.use[d] ? number(names[d], arg[5 + d]) : 0.0;
  }
  if (!cfg.use[0] && !cfg.use[1] && !cfg.use[2])
    error->all(FLERR, "Fix spring/mdp: x, y and z are all NULL: the spring would act in no dimension");
  cfg.r0 = number("R0", arg[8]);
  if (cfg.r0 < 0.0) error->all(FLERR, "Fix spring/mdp: R0 must be >= 0.0");
  int k = 9;
  while (k < narg) {
    const std::string key = arg[k];
    if (key == "vel") {
      if (k + 3 >= narg) error->all(FLERR, "Illegal fix spring/mdp command: vel needs vx vy vz");
      cfg.vel[0] = number("vx", arg[k + 1]);
      cfg.vel[1] = number("vy", arg[k + 2]);
      cfg.vel[2] = number("vz", arg[k + 3]);
      k += 4;
    } else
      error->all(FLERR, "Illegal fix spring/mdp command: unknown keyword " + key);
  }
  vector_flag = 1;
  size_vector = 4;
#ifndef MINILMP_LAMMPS_HOST_API_H
  scalar_flag = 1; // (thermo f_ID under LAMMPS; the mini-host's Fix prints compute_scalar() without these)
  global_freq = 1;
  extscalar = extvector = 1;
#endif
  census();
}

// LAMMPS lets a spring pull on atoms no integrator moves; here the force on them would change nothing, silently, while
// their mass still counts in M: refused in init() with the count, as fix heat/mdp refuses it
void FixSpringMDP::init()
{
  if (comm->nprocs > 1) error->all(FLERR, "Fix spring/mdp runs on one MPI rank only (its sums are taken on one device)");
  int n = 0;
  Fix *nve = walk({"nvt/mdp", "heat/mdp"}, std::string(id) + " cannot run next to fix ",
                  "): springs run under fix nve/mdp, with or without fix langevin/mdp and fix indent/mdp; unfix one of them",
                  "the device's springs need fix nve/mdp as the time integrator",
                  "Fix spring/mdp requires fix nve/mdp with bricks yes as the time integrator", n);
  MdpSprings *block = static_cast<MdpSprings *>(handover(nve, "springs"));
  int dim = 0;
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks_want", dim)); // (its init() may run behind this one)
  if (!bricks) error->all(FLERR, "Fix spring/mdp: this fix nve/mdp does not take springs");
  if (!*bricks)
    error->all(FLERR, std::string("Fix spring/mdp: fix ") + nve->id +
                          " runs in the host-linked mode, where the host keeps atom->image itself: use fix spring (or run the fix with bricks yes)");
  populated();
  inside(nve, "spring");
  block->count = n;
  block->cfg[slot] = cfg;
  block->bit[slot] = igroup == 0 ? 0 : groupbit; // (group all: every owned atom, no mask needed)
}

// FixSpring::compute_scalar: the spring's energy
double FixSpringMDP::compute_scalar()
{
  read(mdp_spring_state, last, true);
  return last[0];
}

// FixSpring::compute_vector: ftotal
double FixSpringMDP::compute_vector(int n)
{
  if (n < 0 || n > 3) return 0.0;
  read(mdp_spring_state, last, true);
  return last[1 + n];
}
