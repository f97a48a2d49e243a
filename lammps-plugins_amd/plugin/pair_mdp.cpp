/* ------------------------------------------------------------------------------------------------
   The shared part of the MI355X pair adapters -- see pair_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "pair_mdp.h"
#include "mdp_brick.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "memory.h"
#include "neigh_list.h"
#include "neighbor.h"

#include <cstring>

using namespace LAMMPS_NS;

PairMDP::PairMDP(LAMMPS *lmp, const char *name_, int style_id_)
    : Pair(lmp), name(name_), style_id(style_id_), overflow_is_neigh_one(false), dev(nullptr), nve_linked(0), nve_mask(0), bricks(nullptr),
      bricks_ev(0), nall_uploaded(-1)
{
}

PairMDP::~PairMDP()
{
  if (dev) mdp_destroy(dev);
  if (allocated) {
    memory->destroy(setflag);
    memory->destroy(cutsq);
    if (ghostneigh) memory->destroy(cutghost);
    delete[] map;
    map = nullptr;
  }
}

void PairMDP::fail_one(int code, const char *what)
{
  std::string msg = prefix() + ": " + what + " failed";
  if (code == MDP_EOVERFLOW && overflow_is_neigh_one) msg = "Neighbor list overflow, boost neigh_modify one";
  if (dev) msg += std::string(": ") + mdp_last_error(dev);
  error->one(FLERR, msg);
}

bool PairMDP::open_device()
{
  if (dev) return false;
  if (mdp_device_count() <= 0) error->all(FLERR, prefix() + " needs a HIP device; there is no CPU fallback");
  if (mdp_create(&dev, mdp_device_of_rank(comm->me)) != MDP_OK) error->one(FLERR, prefix() + ": cannot create a device context");
  return true;
}

void PairMDP::allocate()
{
  allocated = 1;
  const int n = atom->ntypes;
  memory->create(setflag, n + 1, n + 1, "pair:setflag");
  for (int i = 1; i <= n; i++)
    for (int j = i; j <= n; j++) setflag[i][j] = 0;
  memory->create(cutsq, n + 1, n + 1, "pair:cutsq");
  if (ghostneigh) memory->create(cutghost, n + 1, n + 1, "pair:cutghost");
  delete[] map;
  map = new int[n + 1];
  for (int i = 0; i <= n; i++) map[i] = -1;
}

void PairMDP::settings(int narg, char ** /*arg*/)
{
  if (narg != 0) error->all(FLERR, "Illegal pair_style command");
}

// pair_coeff * * file el_1 ... el_ntypes
void PairMDP::coeff_args(int narg, char **arg)
{
  if (!allocated) allocate();
  if (narg != 3 + atom->ntypes) error->all(FLERR, "Incorrect args for pair coefficients");
  if (strcmp(arg[0], "*") != 0 || strcmp(arg[1], "*") != 0) error->all(FLERR, "Incorrect args for pair coefficients");
}

// ... once map[] is filled: the type pairs this style covers (and, given the elements' masses, the types' masses)
void PairMDP::coeff_setflags(const double *element_mass)
{
  const int n = atom->ntypes;
  int count = 0;
  for (int i = 1; i <= n; i++)
    for (int j = i; j <= n; j++) {
      setflag[i][j] = 0;
      if (map[i] >= 0 && map[j] >= 0) {
        setflag[i][j] = 1;
        if (i == j && element_mass) atom->set_mass(FLERR, i, element_mass[map[i]]);
        count++;
      }
    }
  if (count == 0) error->all(FLERR, "Incorrect args for pair coefficients");
}

bool PairMDP::linked() const { return nve_linked && comm->nprocs == 1; }

// host mode, before the forces: box, then -- on the steps on which the host rebuilt its list (atoms may have migrated /
// been re-sorted) -- atoms, lists and, linked to fix nve/mdp, velocities; on the other steps the positions, unless the
// device moved the atoms itself (linked: mdp_hnve_initial).  Returns linked().
bool PairMDP::upload_host(const HostUpload &u)
{
  const int nlocal = atom->nlocal, nall = atom->nlocal + atom->nghost;
  const bool linked = this->linked();
  int rc = mdp_set_box_host(dev, u.box);
  if (rc != MDP_OK) fail_one(rc, "box");
  if (neighbor->ago == 0 || nall != nall_uploaded) {
    rc = mdp_set_atoms_host(dev, nlocal, atom->nghost, nall ? atom->x[0] : nullptr, atom->type, atom->tag, atom->ntypes, u.map);
    if (rc != MDP_OK) fail_one(rc, "atom upload");
    if (u.inum_is_nlocal && list->inum != nlocal) error->one(FLERR, prefix() + ": neighbor list does not match nlocal");
    if (u.host_rows) {
      rc = mdp_set_neighbors_host(dev, list->inum, u.gnum, list->ilist, list->numneigh, list->firstneigh, neighbor->skin);
      if (rc != MDP_OK) fail_one(rc, "neighbor list upload");
    } else {
      // the device builds its own lists from the positions; the host's list (requested in init_style for API parity and
      // for the ghost shell it implies) only contributes its skin ...
      rc = mdp_set_skin(dev, neighbor->skin);
      if (rc != MDP_OK) fail_one(rc, "skin upload");
      // ... which is only the reference's result when the host's list is the plain geometric one: the reference walks the
      // host's entries, so exclusions or special bonds must stop the run
      rc = u.check(dev, list->inum, list->ilist, list->numneigh, list->firstneigh, u.check_cut);
      if (rc != MDP_OK) fail_one(rc, "neighbor list check");
    }
    nall_uploaded = nall;
    // fix nve/mdp integrates on the device: the velocities go with the atoms (the host's are current on this step)
    if (linked) {
      rc = mdp_hnve_upload_v(dev, nlocal ? atom->v[0] : nullptr);
      if (rc != MDP_OK) fail_one(rc, "velocity upload");
      if (nve_mask) { // ... and, when the fix (or its thermostat) acts on a group, atom->mask
        static const int none = 0;
        rc = mdp_hnve_set_mask(dev, nlocal ? atom->mask : &none);
        if (rc != MDP_OK) fail_one(rc, "mask upload");
      }
    }
  } else if (!linked) {
    rc = mdp_set_positions_host(dev, nall ? atom->x[0] : nullptr);
    if (rc != MDP_OK) fail_one(rc, "position upload");
  }
  return linked;
}

// fix nve/mdp on its bricks (several ranks, or `bricks yes`): the step was opened by its initial_integrate on the fix's
// own context (integrate, reneighbor or start the halo, what needs no remote ghost); this is the rest of the step -- for
// aeam fp out and the ghosts' three-body forces back between the bricks on the device, not through pack_forward_comm /
// Comm::reverse_comm.  The host's atom arrays are not read and not written; energy and virial of this rank's atoms on
// the steps that ask.
void PairMDP::compute_bricks()
{
  // per-atom tallies stay on the brick for a reader on the device (compute heatflux/mdp): only on a step the fix opened
  // for them (bit 4: every compute that asks for them is such a reader)
  const int at = (bricks_ev & 4) ? 1 : 0;
  if ((eflag_atom || vflag_atom) && !at)
    error->all(FLERR, prefix() + ": per-atom energy / virial is not available while fix nve/mdp keeps the atoms on its bricks");
  const int want = (eflag_global || vflag_global) ? 1 : 0;
  if (want && !(bricks_ev & 1)) error->all(FLERR, prefix() + ": energy / virial asked for on a step fix nve/mdp opened without them");
  const int ev = (bricks_ev & 1) ? 1 : 0, ef = ev | (at ? 2 : 0), vf = ev | (at ? 4 : 0);
  int rc;
  if (bricks_ev & 2) { // one rank (`bricks yes`): no exchange to wait for -- compute, then the half-kick now or with the next step's
    rc = mdp_md_compute(bricks, ef, vf);
    if (rc == MDP_OK) rc = ev ? mdp_md_final_integrate(bricks) : mdp_md_defer_final(bricks);
  } else
    rc = mdp_dd_comm_step_end(bricks, ef, vf, ev ? 0 : 1);
  if (rc != MDP_OK) error->one(FLERR, prefix() + ": " + mdp_last_error(bricks));
  if (!want) return;
  double t[9];
  if (mdp_md_thermo(bricks, t) != MDP_OK) error->one(FLERR, prefix() + ": " + mdp_last_error(bricks));
  if (eflag_global) eng_vdwl = t[1];
  if (vflag_global)
    for (int k = 0; k < 6; k++) virial[k] = t[2 + k];
}

void *PairMDP::extract(const char *str, int &dim)
{
  // what fix nve/mdp needs of the style: its device context and the switch that keeps x, v and f there ...
  dim = 0;
  if (strcmp(str, "mdp_ctx") == 0) return (void *) &dev;
  if (strcmp(str, "mdp_nve_linked") == 0) return (void *) &nve_linked;
  if (strcmp(str, "mdp_nve_mask") == 0) return (void *) &nve_mask; // (the fix acts on a group: atom->mask goes up with the velocities)
  // ... and where the fix (or minimize/mdp) runs a brick on a context of its own: which style to set that context up for
  // (the derived classes answer for their parameters)
  if (strcmp(str, "mdp_bricks_ctx") == 0) return (void *) &bricks;
  if (strcmp(str, "mdp_bricks_ev") == 0) return (void *) &bricks_ev;
  if (strcmp(str, "mdp_style") == 0) return (void *) &style_id;
  return nullptr;
}
