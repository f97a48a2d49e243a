/* ------------------------------------------------------------------------------------------------
   ComputeMDP -- see compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_mdp.h"

#include "atom.h"
#include "error.h"
#include "fix.h"
#include "group.h"
#include "modify.h"
#include "update.h"

#include <algorithm>
#include <cstring>
#include <utility>

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

void ComputeMDP::peratom_columns(const int ncols)
{
  peratom_flag = 1;
  peratom_ncols = ncols;
  size_peratom_cols = ncols > 1 ? ncols : 0;
}

void ComputeMDP::read_peratom(mdp_ctx *c, peratom_fn read)
{
  invoked_peratom = update->ntimestep;
  // the read writes one row per owned atom of the BRICK: they must be the host's owned atoms
  long long di[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mdp_dd_info(c, di, nullptr, nullptr) != MDP_OK) fail(c);
  const int n = atom->nlocal, w = peratom_ncols;
  if (di[0] != n)
    error->one(FLERR, "Compute " + name + ": the brick owns " + std::to_string(di[0]) + " atoms and the host " + std::to_string(n) +
                          ": per-atom values are read on output steps (thermo, dump, the last step of a run), when the atoms are home");
  const size_t room = (size_t) (atom->nmax > n ? atom->nmax : n) + 1;
  if (values.size() < room * w) values.assign(room * w, 0.0);
  peratom_tags.assign((size_t) n + 1, 0);
  if (read(c, peratom_tags.data(), values.data()) != MDP_OK) fail(c);
  // The brick's order is the host's on every output step of a run (mdp_brick_to_host has just written the host's arrays); at the
  // setup of a run the host still holds its own order.  Then every row goes to the host's atom with the row's ID; an ID the host
  // does not own, or owns twice, ends the run: no value is ever handed out under a wrong atom.
  int first_off = -1;
  for (int i = 0; i < n && first_off < 0; i++)
    if (peratom_tags[i] != atom->tag[i]) first_off = i;
  if (first_off >= 0) {
    std::vector<std::pair<int, int>> host((size_t) n);
    for (int i = 0; i < n; i++) host[i] = {(int) atom->tag[i], i};
    std::sort(host.begin(), host.end());
    std::vector<double> by_host(values.size(), 0.0);
    std::vector<char> filled((size_t) n, 0);
    for (int r = 0; r < n; r++) {
      const auto at = std::lower_bound(host.begin(), host.end(), std::make_pair(peratom_tags[r], -1));
      if (at == host.end() || at->first != peratom_tags[r] || filled[at->second])
        error->one(FLERR, "Compute " + name + ": the brick's atom " + std::to_string(r) + " has ID " + std::to_string(peratom_tags[r]) +
                              ", which the host " + (at == host.end() || at->first != peratom_tags[r] ? "does not own" : "owns twice") +
                              " (its atom " + std::to_string(first_off) + " has ID " + std::to_string(atom->tag[first_off]) +
                              "): the brick's atoms are not the host's on this step, and no per-atom value is handed out");
      filled[at->second] = 1;
      for (int k = 0; k < w; k++) by_host[(size_t) at->second * w + k] = values[(size_t) r * w + k];
    }
    values.swap(by_host);
  }
  if (w > 1) {
    rows.resize(room);
    for (size_t i = 0; i < room; i++) rows[i] = values.data() + i * w;
    array_atom = rows.data();
  } else
    vector_atom = values.data();
}
