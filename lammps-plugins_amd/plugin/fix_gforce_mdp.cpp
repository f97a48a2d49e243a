/* ------------------------------------------------------------------------------------------------
   fix setforce/mdp, fix addforce/mdp, fix aveforce/mdp -- see fix_gforce_mdp.h.  What runs where:
     constructor        the arguments (refused here, before a device is touched: an unknown or empty group, a variable
                        anywhere, region, every and energy on addforce, NULL on addforce, a bad number, an unknown keyword, a
                        fifth fix of the family)
     init()             the one fix nve/mdp found through modify; a copy of the settings written into this fix's slot of its
                        Fix::extract("mdp_gforces") block (mdp_riders.h).  Refused here: no fix nve/mdp, a host-side time
                        integrator, fix nvt/mdp or fix heat/mdp in the same run, several ranks, atoms of the group that the
                        integrator does not move, addforce without bricks yes, atoms shared with an aveforce/mdp defined
                        before this fix, and the two orders of definition the device cannot reproduce
     the steps          fix nve/mdp's: its setup() switches the family on (mdp_gforce_setup, mdp_gforce_run(beginstep)),
                        behind the springs, in the context the steps run on; its post_run() switches it off
     compute_vector()   the total force on the group before the fix acted, compute_scalar() addforce's energy, read from
                        the context of the run under way, once per step
   What it shares with the other fixes that ride on fix nve/mdp is FixRiderMDP's (fix_rider_mdp.h).
-------------------------------------------------------------------------------------------------- */
#include "fix_gforce_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "group.h"
#include "modify.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

static const char *const usage_set = "Illegal fix setforce/mdp command: fix ID group setforce/mdp fx fy fz (a number or NULL each)";
static const char *const usage_add = "Illegal fix addforce/mdp command: fix ID group addforce/mdp fx fy fz";
static const char *const usage_ave = "Illegal fix aveforce/mdp command: fix ID group aveforce/mdp fx fy fz (a number or NULL each)";

FixGforceMDP::FixGforceMDP(LAMMPS *lmp, int narg, char **arg, int kind, const char *name_, const char *usage)
    : FixRiderMDP(lmp, narg, arg, name_, MDP_GFORCE_MAX, "mdp_gforces", 4, usage, "there is no atom to act on",
                  {"setforce/mdp", "addforce/mdp", "aveforce/mdp"})
{
  memset(&cfg, 0, sizeof cfg);
  cfg.kind = kind;
  const std::string head = "Illegal fix " + name + " command: ";
  for (int k = 3; k < narg; k++) // (a variable is named as such wherever it stands, before anything else is said)
    if (strncmp(arg[k], "v_", 2) == 0)
      error->all(FLERR, "Fix " + name + ": a variable as an argument is not supported (" + arg[k] + "); the values are constants");
  if (narg < 6) error->all(FLERR, usage);
  const char *names[3] = {"fx", "fy", "fz"};
  for (int d = 0; d < 3; d++) {
    cfg.use[d] = strcmp(arg[3 + d], "NULL") != 0;
    if (!cfg.use[d] && kind == MDP_GFORCE_ADD)
      error->all(FLERR, "Fix addforce/mdp: " + std::string(names[d]) + " is NULL; addforce takes three numbers (0.0 adds nothing)");
    cfg.f[d] = cfg.use[d] ? mdp_number(error, head, names[d], arg[3 + d], true) : 0.0;
  }
  for (int k = 6; k < narg; k++) {
    const std::string key = arg[k];
    if (key == "region") error->all(FLERR, "Fix " + name + ": region is not supported; the fix acts on every atom of its group");
    if (kind == MDP_GFORCE_ADD && (key == "every" || key == "energy"))
      error->all(FLERR, "Fix addforce/mdp: " + key + " is not supported; the force is added on every step and is constant");
    error->all(FLERR, head + "unknown keyword " + key);
  }
  vector_flag = 1;
  size_vector = 3;
#ifndef MINILMP_LAMMPS_HOST_API_H
  scalar_flag = kind == MDP_GFORCE_ADD; // (thermo f_ID under LAMMPS; the mini-host's Fix prints compute_scalar() without these)
  global_freq = 1;
  extscalar = extvector = 1;
#endif
  census();
}

FixSetForceMDP::FixSetForceMDP(LAMMPS *lmp, int narg, char **arg) : FixGforceMDP(lmp, narg, arg, MDP_GFORCE_SET, "setforce/mdp", usage_set) {}
FixAddForceMDP::FixAddForceMDP(LAMMPS *lmp, int narg, char **arg) : FixGforceMDP(lmp, narg, arg, MDP_GFORCE_ADD, "addforce/mdp", usage_add) {}
FixAveForceMDP::FixAveForceMDP(LAMMPS *lmp, int narg, char **arg) : FixGforceMDP(lmp, narg, arg, MDP_GFORCE_AVE, "aveforce/mdp", usage_ave) {}

double FixGforceMDP::shared_with(const Fix *other) const
{
  double mine = 0.0, all = 0.0;
  for (int a = 0; a < atom->nlocal; a++)
    if ((atom->mask[a] & groupbit) && (atom->mask[a] & other->groupbit)) mine += 1.0;
  MPI_Allreduce(&mine, &all, 1, MPI_DOUBLE, MPI_SUM, world);
  return all;
}

// LAMMPS lets these fixes act on atoms no integrator moves; here the force on them would change nothing, silently, while
// they still count in the sums: refused in init() with the count, as fix spring/mdp refuses it
void FixGforceMDP::init()
{
  if (comm->nprocs > 1) error->all(FLERR, "Fix " + name + " runs on one MPI rank only (its sums are taken on one device)");
  int n = 0;
  Fix *nve = walk({"nvt/mdp", "heat/mdp"}, std::string(id) + " cannot run next to fix ",
                  "): the fix runs under fix nve/mdp, with or without fix langevin/mdp, fix indent/mdp and fix spring/mdp; unfix one of them",
                  "the device's group forces need fix nve/mdp as the time integrator",
                  ("Fix " + name + " requires fix nve/mdp as the time integrator").c_str(), n);
  MdpGforces *block = static_cast<MdpGforces *>(handover(nve, "group forces"));
  if (cfg.kind == MDP_GFORCE_ADD) {
    int dim = 0;
    const int *bricks = static_cast<int *>(nve->extract("mdp_bricks_want", dim)); // (its init() may run behind this one)
    if (!bricks || !*bricks)
      error->all(FLERR, std::string("Fix addforce/mdp: fix ") + nve->id +
                            " runs in the host-linked mode, where the host keeps atom->image itself: use fix addforce (or run the fix with bricks yes)");
  }
  populated();
  inside(nve, "force");
  // the order of definition.  Behind this fix in Modify's list: `later`
  bool later = false;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (f == this) {
      later = true;
      continue;
    }
    const std::string other = f->style;
    // an average needs its whole group before what follows it is known: nothing behind an aveforce/mdp shares its atoms
    if (!later && other == "aveforce/mdp") {
      const double shared = shared_with(f);
      if (shared > 0.0)
        error->all(FLERR, "Fix " + name + ": fixes " + f->id + " (aveforce/mdp) and " + id + " share " + std::to_string((long long) shared) +
                              " atoms (groups " + group->names[f->igroup] + " and " + group->names[igroup] +
                              "); a fix defined after an aveforce/mdp must not share atoms with it: define " + id + " first");
    }
    if (cfg.kind == MDP_GFORCE_ADD) continue; // (adding commutes with the other forces up to rounding)
    // the device runs this fix behind the indenters and the springs and in front of the Langevin force
    const bool pushes = other == "indent/mdp" || other == "spring/mdp";
    if ((later && pushes) || (!later && other == "langevin/mdp")) {
      const double shared = shared_with(f);
      if (shared > 0.0)
        error->all(FLERR, "Fix " + name + ": " + id + " is defined " + (later ? "before" : "after") + " fix " + f->id + " (" + other + "), which shares " +
                              std::to_string((long long) shared) + " atoms with it; the device applies " + name + (later ? " behind " : " in front of ") +
                              other + ": define " + (later ? std::string(f->id) + " first, then " + id : std::string(id) + " first, then " + f->id));
    }
  }
  block->count = n;
  block->cfg[slot] = cfg;
  block->bit[slot] = igroup == 0 ? 0 : groupbit; // (group all: every owned atom, no mask needed)
}

// FixAddForce::compute_scalar: the potential energy of the added force; 0 for the other two styles
double FixGforceMDP::compute_scalar()
{
  read(mdp_gforce_state, last, true);
  return last[0];
}

// compute_vector of all three: the total force on the group before the fix acted
double FixGforceMDP::compute_vector(int n)
{
  if (n < 0 || n > 2) return 0.0;
  read(mdp_gforce_state, last, true);
  return last[1 + n];
}
