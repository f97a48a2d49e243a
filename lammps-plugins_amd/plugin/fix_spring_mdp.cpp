/* ------------------------------------------------------------------------------------------------
   fix spring/mdp -- see fix_spring_mdp.h.  What runs where:
     constructor        the arguments (refused here, before a device is touched: an unknown or empty group, couple, a
                        variable anywhere, bad or negative K or R0, x, y and z all NULL, an unknown keyword, a fifth
                        spring/mdp)
     init()             the one fix nve/mdp found through modify; a copy of the settings written into this fix's slot of its
                        Fix::extract("mdp_springs") block (mdp_spring.h).  Refused here: no fix nve/mdp, one without bricks
                        yes, a host-side time integrator, fix nvt/mdp or fix heat/mdp in the same run, several ranks, atoms
                        of the group that the integrator does not move
     the steps          fix nve/mdp's: its setup() switches the springs on (mdp_spring_setup, mdp_spring_run(beginstep)),
                        behind the indenters, in the context the steps run on; its post_run() switches them off
     compute_scalar()   the spring's energy, compute_vector(0..3) ftotal, read through the context fix nve/mdp exposes
                        (Fix::extract("mdp_spring_ctx"))
-------------------------------------------------------------------------------------------------- */
#include "fix_spring_mdp.h"
#include "mdp_args.h"
#include "mdp_spring.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "group.h"
#include "modify.h"
#include "update.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

double FixSpringMDP::number(const char *what, const char *s)
{
  if (strncmp(s, "v_", 2) == 0)
    error->all(FLERR, std::string("Fix spring/mdp: a variable as ") + what + " is not supported (" + s + "); a moving tether point takes vel vx vy vz");
  return mdp_number(error, "Illegal fix spring/mdp command: ", what, s, true);
}

FixSpringMDP::FixSpringMDP(LAMMPS *lmp, int narg, char **arg) : Fix(lmp, narg, arg)
{
  memset(&cfg, 0, sizeof cfg);
  const char *usage = "Illegal fix spring/mdp command: fix ID group spring/mdp tether K x y z R0 [vel vx vy vz]";
  if (narg < 4) error->all(FLERR, usage);
  if (igroup < 0)
    error->all(FLERR, std::string("Fix spring/mdp requires group all or a group defined by the group command: could not find fix group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Fix spring/mdp: group ") + arg[1] + " is empty: there is no centre of mass to pull on");
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
  int earlier = 0;
  for (int i = 0; i < modify->nfix; i++) // (a fix with this ID is replaced by this one: it does not count)
    if (strcmp(modify->fix[i]->style, "spring/mdp") == 0 && strcmp(modify->fix[i]->id, id) != 0) earlier++;
  if (earlier + 1 > MDP_SPRING_MAX) too_many(earlier + 1);
}

void FixSpringMDP::too_many(int n)
{
  error->all(FLERR, std::string("Fix spring/mdp: ") + id + " is spring/mdp fix number " + std::to_string(n) + "; fix nve/mdp takes up to " +
                        std::to_string(MDP_SPRING_MAX) + " of them");
}

int FixSpringMDP::setmask() { return 0; } // (the pass runs inside fix nve/mdp's device steps)

Fix *FixSpringMDP::integrator() const
{
  for (int i = 0; i < modify->nfix; i++)
    if (strcmp(modify->fix[i]->style, "nve/mdp") == 0) return modify->fix[i];
  return nullptr;
}

// LAMMPS lets a spring pull on atoms no integrator moves; here the force on them would change nothing, silently, while
// their mass still counts in M: refused with the count, as fix heat/mdp refuses it
void FixSpringMDP::inside(Fix *nve)
{
  if (igroup == nve->igroup || nve->igroup == 0) return;
  long outside = 0;
  for (int i = 0; i < atom->nlocal; i++)
    if ((atom->mask[i] & groupbit) && !(atom->mask[i] & nve->groupbit)) outside++;
  if (outside)
    error->one(FLERR, std::string("Fix spring/mdp: group ") + group->names[igroup] + " has " + std::to_string(outside) +
                          " atoms outside group " + group->names[nve->igroup] + " of fix " + nve->id +
                          " (nve/mdp): the spring acts on atoms the integrator moves");
}

void FixSpringMDP::init()
{
  if (comm->nprocs > 1) error->all(FLERR, "Fix spring/mdp runs on one MPI rank only (its sums are taken on one device)");
  read_step = -1; // (a new run: its setup state is not the last run's last)
  Fix *nve = nullptr;
  int n = 0;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "spring/mdp") == 0) { // (this fix among them: its slot is its position in the list)
      if (f == this) slot = n;
      n++;
      continue;
    }
    if (strcmp(f->style, "nvt/mdp") == 0 || strcmp(f->style, "heat/mdp") == 0)
      error->all(FLERR, std::string("Fix spring/mdp: fix ") + id + " cannot run next to fix " + f->id + " (" + f->style +
                            "): springs run under fix nve/mdp, with or without fix langevin/mdp and fix indent/mdp; unfix one of them");
    if (strcmp(f->style, "nve/mdp") == 0) nve = f;
    else if (f->time_integrate)
      error->all(FLERR, std::string("Fix spring/mdp: fix ") + f->id + " (" + f->style +
                            ") integrates on the host; the device's springs need fix nve/mdp as the time integrator");
  }
  if (!nve) error->all(FLERR, "Fix spring/mdp requires fix nve/mdp with bricks yes as the time integrator");
  if (n > MDP_SPRING_MAX) too_many(n);
  int dim = 0;
  MdpSprings *block = static_cast<MdpSprings *>(nve->extract("mdp_springs", dim));
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks_want", dim)); // (its init() may run behind this one)
  if (!block || !bricks) error->all(FLERR, "Fix spring/mdp: this fix nve/mdp does not take springs");
  if (!*bricks)
    error->all(FLERR, std::string("Fix spring/mdp: fix ") + nve->id +
                          " runs in the host-linked mode, where the host keeps atom->image itself: use fix spring (or run the fix with bricks yes)");
  if ((igroup == 0 ? (double) atom->natoms : (double) group->count(igroup)) < 1.0)
    error->all(FLERR, std::string("Fix spring/mdp: group ") + group->names[igroup] + " is empty: there is no centre of mass to pull on");
  inside(nve);
  block->count = n;
  block->cfg[slot] = cfg;
  block->bit[slot] = igroup == 0 ? 0 : groupbit; // (group all: every owned atom, no mask needed)
}

void FixSpringMDP::read()
{
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **c = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_spring_ctx", dim)) : nullptr;
  if (!c || !*c) return; // (between runs: what the last read returned)
  if (read_step == update->ntimestep) return; // (one blocking read per step serves f_ID and f_ID[1..4])
  double st[MDP_SPRING_STATE_LEN];
  if (mdp_spring_state(*c, slot, st) != MDP_OK) error->one(FLERR, std::string("Fix spring/mdp: ") + mdp_last_error(*c));
  for (int k = 0; k < 5; k++) last[k] = st[k];
  read_step = update->ntimestep;
}

// FixSpring::compute_scalar: the spring's energy
double FixSpringMDP::compute_scalar()
{
  read();
  return last[0];
}

// FixSpring::compute_vector: ftotal
double FixSpringMDP::compute_vector(int n)
{
  if (n < 0 || n > 3) return 0.0;
  read();
  return last[1 + n];
}
