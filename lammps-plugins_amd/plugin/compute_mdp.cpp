/* ------------------------------------------------------------------------------------------------
   ComputeMDP -- see compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_mdp.h"

#include "error.h"
#include "fix.h"
#include "group.h"
#include "modify.h"

#include <cstring>

using namespace LAMMPS_NS;

ComputeMDP::ComputeMDP(LAMMPS *lmp, int narg, char **arg, const char *name_, const char *empty_tail)
    : Compute(lmp, narg, arg), name(name_), head("Illegal compute " + name + " command: "), sent_to(nullptr), sent_serial(0)
{
  if (igroup < 0)
    error->all(FLERR, "Compute " + name + " requires group all or a group defined by the group command: could not find compute group ID " + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0) error->all(FLERR, "Compute " + name + ": group " + arg[1] + " is empty: " + empty_tail);
}

void ComputeMDP::fail(mdp_ctx *c) const { error->one(FLERR, "Compute " + name + ": " + (c ? mdp_last_error(c) : "no device context")); }

// the one time integrator of this plugin family: fix nve/mdp, or fix nvt/mdp that is built on it
Fix *ComputeMDP::integrator() const
{
  Fix *found = nullptr;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "nve/mdp") != 0 && strcmp(f->style, "nvt/mdp") != 0) continue;
    if (found) error->all(FLERR, "Compute " + name + ": fixes " + found->id + " and " + f->id + " both integrate on the device; it reads one run's context");
    found = f;
  }
  return found;
}

void ComputeMDP::require_bricks(const char *hint) const
{
  Fix *nve = integrator();
  if (!nve) error->all(FLERR, "Compute " + name + " requires fix nve/mdp (or fix nvt/mdp) with bricks yes as the time integrator");
  int dim = 0;
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks", dim));
  if (!bricks || !nve->extract("mdp_steps_ctx", dim)) error->all(FLERR, "Compute " + name + ": fix " + nve->id + " does not expose its run's context");
  if (!*bricks) error->all(FLERR, "Compute " + name + ": fix " + nve->id + " runs in the host-linked mode, " + hint);
}

mdp_ctx *ComputeMDP::run_context() const
{
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **slot = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_steps_ctx", dim)) : nullptr;
  if (!slot || !*slot) error->all(FLERR, "Compute " + name + ": no run of fix nve/mdp is under way; the atoms are on the device only during one");
  return *slot;
}

bool ComputeMDP::sent(mdp_ctx *c, info_fn info)
{
  long long w[4] = {0, 0, 0, 0};
  if (info(c, w) != MDP_OK) fail(c);
  return c == sent_to && w[0] && w[3] == sent_serial;
}

void ComputeMDP::record(mdp_ctx *c, info_fn info)
{
  long long w[4] = {0, 0, 0, 0};
  if (info(c, w) != MDP_OK) fail(c);
  sent_to = c;
  sent_serial = w[3];
}

void ComputeMDP::global_array(const long long nrows, const int ncols)
{
  array_flag = 1;
  extarray = 0;
  size_array_rows = (int) nrows;
  size_array_cols = ncols;
  values.assign((size_t) nrows * ncols, 0.0);
  rows.resize((size_t) nrows);
  for (size_t b = 0; b < rows.size(); b++) rows[b] = values.data() + b * ncols;
  array = rows.data();
}
