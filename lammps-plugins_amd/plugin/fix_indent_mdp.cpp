/* ------------------------------------------------------------------------------------------------
   fix indent/mdp -- see fix_indent_mdp.h.  What runs where:
     constructor        the arguments (refused here, before a device is touched: an unknown or empty group, a variable
                        anywhere, bad numbers, side on a plane, an unknown keyword, units other than box or none at all, a
                        cylinder that moves along its axis, a box with a non-periodic dimension, a fifth indent/mdp)
     init()             the one fix nve/mdp found through modify; a copy of the settings written into this fix's slot of its
                        Fix::extract("mdp_indenters") block (mdp_riders.h).  Refused here: no fix nve/mdp, a host-side time
                        integrator, a non-periodic dimension, fix nvt/mdp or fix heat/mdp in the same run, several ranks
     the steps          fix nve/mdp's: its setup() switches the indenters on (mdp_indent_setup, mdp_indent_run(beginstep))
                        in the context the steps run on, its post_run() switches them off
     compute_scalar()   the indenter's energy, compute_vector(0..2) the force on it, read from the context of the run under
                        way, once per step
   What it shares with the other fixes that ride on fix nve/mdp is FixRiderMDP's (fix_rider_mdp.h).
-------------------------------------------------------------------------------------------------- */
#include "fix_indent_mdp.h"
#include "mdp_args.h"

#include "comm.h"
#include "domain.h"
#include "error.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

double FixIndentMDP::number(const char *what, const char *s)
{
  if (strncmp(s, "v_", 2) == 0)
    error->all(FLERR, std::string("Fix indent/mdp: a variable as ") + what + " is not supported (" + s + "); a moving indenter takes vel vx vy vz");
  return mdp_number(error, "Illegal fix indent/mdp command: ", what, s, true);
}

static int indent_dim(Error *error, const char *s)
{
  if (strcmp(s, "x") == 0) return 0;
  if (strcmp(s, "y") == 0) return 1;
  if (strcmp(s, "z") == 0) return 2;
  error->all(FLERR, std::string("Illegal fix indent/mdp command: dim must be x, y or z, not ") + s);
  return 0;
}

static const char *const usage = "Illegal fix indent/mdp command: fix ID group indent/mdp K sphere x y z R | cylinder dim c1 c2 R | plane dim pos lo|hi "
                                 "[side in|out] [vel vx vy vz] units box";

FixIndentMDP::FixIndentMDP(LAMMPS *lmp, int narg, char **arg)
    : FixRiderMDP(lmp, narg, arg, "indent/mdp", MDP_INDENT_MAX, "mdp_indenters", 5, usage, "there is no atom to push on")
{
  memset(&cfg, 0, sizeof cfg);
  for (int k = 3; k < narg; k++) // (a variable is named as such wherever it stands, before anything else is said)
    if (strncmp(arg[k], "v_", 2) == 0) number("an argument", arg[k]);
  cfg.k = number("K", arg[3]);
  if (cfg.k < 0.0) error->all(FLERR, "Fix indent/mdp: K must be >= 0.0");
  int k = 5;
  const std::string shape = arg[4];
  if (shape == "sphere") {
    if (narg < 9) error->all(FLERR, usage);
    cfg.shape = MDP_INDENT_SPHERE;
    cfg.c[0] = number("x", arg[5]);
    cfg.c[1] = number("y", arg[6]);
    cfg.c[2] = number("z", arg[7]);
    cfg.r = number("R", arg[8]);
    k = 9;
  } else if (shape == "cylinder") {
    if (narg < 9) error->all(FLERR, usage);
    cfg.shape = MDP_INDENT_CYLINDER;
    cfg.dim = indent_dim(error, arg[5]);
    cfg.c[cfg.dim == 0 ? 1 : 0] = number("c1", arg[6]); // (x: y z; y: x z; z: x y, as FixIndent)
    cfg.c[cfg.dim == 2 ? 1 : 2] = number("c2", arg[7]);
    cfg.r = number("R", arg[8]);
    k = 9;
  } else if (shape == "plane") {
    if (narg < 8) error->all(FLERR, usage);
    cfg.shape = MDP_INDENT_PLANE;
    cfg.dim = indent_dim(error, arg[5]);
    cfg.c[cfg.dim] = number("pos", arg[6]);
    if (strcmp(arg[7], "lo") == 0) cfg.side = 0;
    else if (strcmp(arg[7], "hi") == 0) cfg.side = 1;
    else error->all(FLERR, std::string("Illegal fix indent/mdp command: a plane takes lo or hi, not ") + arg[7]);
    k = 8;
  } else
    error->all(FLERR, "Illegal fix indent/mdp command: unknown shape " + shape + " (sphere, cylinder or plane)");
  if (cfg.shape != MDP_INDENT_PLANE && cfg.r < 0.0) error->all(FLERR, "Fix indent/mdp: R must be >= 0.0");
  bool box = false;
  while (k < narg) {
    const std::string key = arg[k];
    if (key == "side") {
      if (k + 1 >= narg) error->all(FLERR, "Illegal fix indent/mdp command: side needs in or out");
      if (cfg.shape == MDP_INDENT_PLANE) error->all(FLERR, "Fix indent/mdp: keyword side is not for a plane, whose side is lo or hi");
      if (strcmp(arg[k + 1], "in") == 0) cfg.side = 1;
      else if (strcmp(arg[k + 1], "out") == 0) cfg.side = 0;
      else error->all(FLERR, std::string("Illegal fix indent/mdp command: side takes in or out, not ") + arg[k + 1]);
      k += 2;
    } else if (key == "vel") {
      if (k + 3 >= narg) error->all(FLERR, "Illegal fix indent/mdp command: vel needs vx vy vz");
      cfg.vel[0] = number("vx", arg[k + 1]);
      cfg.vel[1] = number("vy", arg[k + 2]);
      cfg.vel[2] = number("vz", arg[k + 3]);
      k += 4;
    } else if (key == "units") {
      if (k + 1 >= narg) error->all(FLERR, "Illegal fix indent/mdp command: units needs a value");
      if (strcmp(arg[k + 1], "box") != 0)
        error->all(FLERR, std::string("Fix indent/mdp: units ") + arg[k + 1] + " is not supported; write `units box` and give lengths in box units");
      box = true;
      k += 2;
    } else
      error->all(FLERR, "Illegal fix indent/mdp command: unknown keyword " + key);
  }
  if (!box)
    error->all(FLERR, "Fix indent/mdp: `units box` must be given; units lattice, LAMMPS' default for fix indent, is not supported");
  if (cfg.shape == MDP_INDENT_CYLINDER && cfg.vel[cfg.dim] != 0.0)
    error->all(FLERR, "Fix indent/mdp: a cylinder cannot move along its axis");
  vector_flag = 1;
  size_vector = 3;
#ifndef MINILMP_LAMMPS_HOST_API_H
  scalar_flag = 1; // (thermo f_ID under LAMMPS; the mini-host's Fix prints compute_scalar() without these)
  global_freq = 1;
  extscalar = extvector = 1;
#endif
  periodic_or_refuse();
  census();
}

// The library takes the box of a host-linked context to be periodic in all three dimensions (mdp_set_box_host carries no
// boundary flags) and a brick needs a periodic box anyway: Domain::minimum_image would wrap across a face that LAMMPS
// leaves alone, and an atom at the far end of a non-periodic box would feel the indenter through it.  Refused, not guessed.
void FixIndentMDP::periodic_or_refuse()
{
  const char *dims = "xyz";
  const int per[3] = {domain->xperiodic, domain->yperiodic, domain->zperiodic};
  for (int d = 0; d < 3; d++)
    if (!per[d])
      error->all(FLERR, std::string("Fix indent/mdp: the box is not periodic in ") + dims[d] +
                            "; the device's minimum image wraps every dimension, so a non-periodic boundary is not supported "
                            "(use a periodic box with vacuum, as examples/in.rebomos-sheet.indent-mdp.mi355x does)");
}

void FixIndentMDP::init()
{
  if (comm->nprocs > 1) error->all(FLERR, "Fix indent/mdp runs on one MPI rank only (its sums are taken on one device)");
  periodic_or_refuse(); // (a `boundary` or `change_box` command may stand behind the fix)
  int n = 0;
  Fix *nve = walk({"nvt/mdp", "heat/mdp"}, std::string(id) + " cannot run next to fix ",
                  "): indenters run under fix nve/mdp, with or without fix langevin/mdp; unfix one of them",
                  "the device's indenters need fix nve/mdp as the time integrator", "Fix indent/mdp requires fix nve/mdp as the time integrator", n);
  MdpIndenters *block = static_cast<MdpIndenters *>(handover(nve, "indenters"));
  populated();
  block->count = n;
  block->cfg[slot] = cfg;
  block->bit[slot] = igroup == 0 ? 0 : groupbit; // (group all: every owned atom, no mask needed)
}

// FixIndent::compute_scalar: the indenter's energy
double FixIndentMDP::compute_scalar()
{
  read(mdp_indent_state, last, true);
  return last[0];
}

// FixIndent::compute_vector: the force on the indenter
double FixIndentMDP::compute_vector(int n)
{
  if (n < 0 || n > 2) return 0.0;
  read(mdp_indent_state, last, true);
  return last[1 + n];
}
