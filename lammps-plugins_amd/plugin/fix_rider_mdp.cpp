/* ------------------------------------------------------------------------------------------------
   FixRiderMDP -- see fix_rider_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "fix_rider_mdp.h"

#include "atom.h"
#include "error.h"
#include "group.h"
#include "modify.h"
#include "update.h"

#include <cstring>

using namespace LAMMPS_NS;

FixRiderMDP::FixRiderMDP(LAMMPS *lmp, int narg, char **arg, const char *name_, int max_, const char *key_, int min_narg,
                         const char *usage, const char *empty_tail_, std::initializer_list<const char *> family_)
    : Fix(lmp, narg, arg), name(name_), max(max_), key(key_), empty_tail(empty_tail_), family(family_.begin(), family_.end())
{
  if (narg < min_narg) error->all(FLERR, usage);
  if (igroup < 0)
    error->all(FLERR, "Fix " + name + " requires group all or a group defined by the group command: could not find fix group ID " + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0) error->all(FLERR, "Fix " + name + ": group " + arg[1] + " is empty: " + empty_tail);
}

Fix *FixRiderMDP::integrator() const
{
  for (int i = 0; i < modify->nfix; i++)
    if (strcmp(modify->fix[i]->style, "nve/mdp") == 0) return modify->fix[i];
  return nullptr;
}

bool FixRiderMDP::kin(const char *style) const
{
  if (name == style) return true;
  for (const std::string &f : family)
    if (f == style) return true;
  return false;
}

std::string FixRiderMDP::kind() const
{
  if (family.empty()) return name;
  std::string s;
  for (size_t k = 0; k < family.size(); k++) s += (k == 0 ? "" : k + 1 == family.size() ? " or " : ", ") + family[k];
  return s;
}

// From the constructor this fix is not in the list yet and is the one behind all it finds; from init() it is in the list,
// and its slot is its position among them.  (LAMMPS constructs a fix before it removes the one whose ID it takes over.)
int FixRiderMDP::census()
{
  int n = 0;
  bool listed = false;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (f == this) {
      listed = true;
      slot = n;
    } else if (!kin(f->style) || strcmp(f->id, id) == 0)
      continue;
    n++;
  }
  if (!listed) n++;
  if (n > max)
    error->all(FLERR, "Fix " + name + ": " + id + " is " + kind() + " fix number " + std::to_string(n) + "; fix nve/mdp takes up to " +
                          std::to_string(max) + " of them");
  return n;
}

// The device's one pass gives an atom one fix of this style (LAMMPS would apply two), so shared atoms are refused.  Every
// such fix before this one in Modify's list is looked at (all of them while this fix is being constructed: it is not in the
// list yet), so each pair is looked at once.
void FixRiderMDP::disjoint()
{
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (f == this) break;
    if (name != f->style || strcmp(f->id, id) == 0) continue;
    double mine = 0.0, shared = 0.0;
    for (int a = 0; a < atom->nlocal; a++)
      if ((atom->mask[a] & groupbit) && (atom->mask[a] & f->groupbit)) mine += 1.0;
    MPI_Allreduce(&mine, &shared, 1, MPI_DOUBLE, MPI_SUM, world);
    if (shared > 0.0)
      error->all(FLERR, "Fix " + name + ": fixes " + f->id + " and " + id + " share " + std::to_string((long long) shared) + " atoms (groups " +
                            group->names[f->igroup] + " and " + group->names[igroup] + "); the groups of several " + name +
                            " fixes must be disjoint");
  }
}

// the fix acts inside the device's steps: an atom it acts on must be one the integrator moves
void FixRiderMDP::inside(Fix *nve, const char *noun)
{
  if (igroup == nve->igroup || nve->igroup == 0) return;
  long outside = 0;
  for (int i = 0; i < atom->nlocal; i++)
    if ((atom->mask[i] & groupbit) && !(atom->mask[i] & nve->groupbit)) outside++;
  if (outside)
    error->one(FLERR, "Fix " + name + ": group " + group->names[igroup] + " has " + std::to_string(outside) + " atoms outside group " +
                          group->names[nve->igroup] + " of fix " + nve->id + " (nve/mdp): the " + noun + " acts on atoms the integrator moves");
}

Fix *FixRiderMDP::walk(std::initializer_list<const char *> refused, const std::string &before, const char *after, const char *host,
                       const char *lacking, int &count)
{
  read_step = -1;    // (a new run: its setup state is not the last run's last)
  Fix *nve = nullptr;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (kin(f->style)) continue;
    for (const char *style : refused)
      if (strcmp(f->style, style) == 0) error->all(FLERR, "Fix " + name + ": fix " + before + f->id + " (" + f->style + after);
    if (strcmp(f->style, "nve/mdp") == 0) nve = f;
    else if (f->time_integrate)
      error->all(FLERR, "Fix " + name + ": fix " + f->id + " (" + f->style + ") integrates on the host; " + host);
  }
  if (!nve) error->all(FLERR, lacking);
  count = census();
  return nve;
}

void *FixRiderMDP::handover(Fix *nve, const char *takes)
{
  int dim = 0;
  void *b = nve->extract(key, dim);
  if (!b) error->all(FLERR, "Fix " + name + ": this fix nve/mdp does not take " + takes);
  return b;
}

double FixRiderMDP::populated()
{
  const double n = igroup == 0 ? (double) atom->natoms : (double) group->count(igroup);
  if (n < 1.0) error->all(FLERR, "Fix " + name + ": group " + group->names[igroup] + " is empty: " + empty_tail);
  return n;
}

// fix nve/mdp keeps one pointer for all it drives: the context of the run under way, null between runs.  A style takes
// part in that run if its block's count, which post_run() clears, is positive.
bool FixRiderMDP::read(state_fn fn, double *out, bool once)
{
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **c = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_steps_ctx", dim)) : nullptr;
  const int *count = nve ? static_cast<int *>(nve->extract(key, dim)) : nullptr;
  if (!c || !*c || !count || *count < 1) return false;
  if (once && read_step == update->ntimestep) return true;
  if (fn(*c, slot, out) != MDP_OK) error->one(FLERR, "Fix " + name + ": " + mdp_last_error(*c));
  read_step = update->ntimestep;
  return true;
}
