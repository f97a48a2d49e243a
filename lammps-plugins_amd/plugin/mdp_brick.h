/* -*- c++ -*- -----------------------------------------------------------------------------------
   The host's atoms as one brick of the library's own decomposition and back: what `fix nve/mdp bricks yes` does around a
   run and `minimize/mdp` around a minimisation -- and, before that, the way to a context of one's own that carries the
   pair style's parameters, on the device every context of a rank lives on.  Free functions over the host's objects, so
   that a Pair, a Fix and a Command (whose Pointers members are protected) share them.
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_BRICK_H
#define MDP_BRICK_H

#include "atom.h"
#include "atom_vec.h"
#include "comm.h"
#include "domain.h"
#include "force.h"
#include "group.h"
#include "neighbor.h"
#include "pair.h"
#include "update.h"

#include "mdpair_hip.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace LAMMPS_NS {

// the device of a rank's contexts: round robin over the devices there are, or what MDP_DEVICE says
inline int mdp_device_of_rank(int me)
{
  const int ndev = mdp_device_count();
  if (const char *env = getenv("MDP_DEVICE")) return atoi(env);
  return ndev > 0 ? me % ndev : 0;
}

inline int mdp_pair_style_id(Pair *pair)
{
  int dim = 0;
  const int *sid = pair ? static_cast<int *>(pair->extract("mdp_style", dim)) : nullptr;
  return sid ? *sid : 0;
}

// a context of the caller's own for the pair style's potential: created on this rank's device unless *ctx is there already,
// then given the style's parameters / tables (Pair::extract).  Failures come back in words for the caller to put its
// own name in front of: `why` for error->all, `failed` (the library step; the reason is mdp_last_error(*ctx), and *ctx
// is null if it could not be created) for error->one.
struct mdp_own_context_result {
  int style_id = 0;             // 1 rebomos, 2 aeam
  const int *map = nullptr;     // rebomos: the style's type -> element map
  const char *why = nullptr, *failed = nullptr;
};

inline mdp_own_context_result mdp_own_context(Pair *pair, int me, mdp_ctx **ctx)
{
  mdp_own_context_result r;
  int dim = 0;
  r.style_id = mdp_pair_style_id(pair);
  if (!r.style_id) {
    r.why = " requires a pair style of this plugin (rebomos or aeam)";
    return r;
  }
  if (!*ctx && mdp_create(ctx, mdp_device_of_rank(me)) != MDP_OK) {
    r.failed = "context";
    return r;
  }
  if (r.style_id == 1) {
    const mdp_rebomos_params *P = static_cast<mdp_rebomos_params *>(pair->extract("mdp_rebomos_params", dim));
    if (!P) r.why = ": the pair style has no parameters yet (pair_coeff)";
    else if (mdp_rebomos_set_params(*ctx, P) != MDP_OK) r.failed = "parameters";
    r.map = static_cast<int *>(pair->extract("mdp_map", dim));
  } else {
    const mdp_aeam_tables *T = static_cast<mdp_aeam_tables *>(pair->extract("mdp_aeam_tables", dim));
    if (!T) r.why = ": the pair style has no tables yet (pair_coeff)";
    else if (mdp_aeam_set_tables(*ctx, T) != MDP_OK) r.failed = "tables";
  }
  return r;
}

// does the host have a group besides `all`?  Then atom->mask says something, and a brick carries it (mdp_md_set_mask)
inline bool mdp_host_has_groups(Group *group) { return group && group->ngroup > 1; }

// this rank's owned atoms (x, v, type, tag as the host holds them) -> the brick of rank comm->me on comm->procgrid:
// mdp_md_setup + mdp_dd_setup.  style_id: 1 rebomos (map: the style's type -> element map), 2 aeam.  with_mask: atom->mask
// goes with the atoms (mdp_md_set_mask) and follows them through every reneighboring and migration.  atom->image always goes
// with them (mdp_md_set_image): the device's remap counts the box vectors it takes off an atom, as Domain::remap does.
// Returns the library's code; the message is mdp_last_error(ctx).
inline int mdp_brick_from_host(mdp_ctx *ctx, int style_id, const int *map, Atom *atom, Domain *domain, Force *force,
                               Neighbor *neighbor, Update *update, Comm *comm, bool with_mask)
{
  const int n = atom->nlocal;
  const double skin = neighbor->skin, cutghost = force->pair->cutforce + skin;
  mdp_md_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.style = style_id;
  cfg.nlocal = n;
  cfg.ntypes = atom->ntypes;
  cfg.skin = skin;
  cfg.dt = update->dt;
  cfg.ftm2v = force->ftm2v;
  cfg.mvv2e = force->mvv2e;
  // provisional bounds (the library sets the brick's at every reneighboring): the box's Cartesian hull + the ghost shell
  const double *h = domain->h; // xprd, yprd, zprd, yz, xz, xy
  cfg.bbox_lo[0] = domain->boxlo[0] + fmin(0.0, h[5]) + fmin(0.0, h[4]) - cutghost - 2.0;
  cfg.bbox_hi[0] = domain->boxlo[0] + h[0] + fmax(0.0, h[5]) + fmax(0.0, h[4]) + cutghost + 2.0;
  cfg.bbox_lo[1] = domain->boxlo[1] + fmin(0.0, h[3]) - cutghost - 2.0;
  cfg.bbox_hi[1] = domain->boxlo[1] + h[1] + fmax(0.0, h[3]) + cutghost + 2.0;
  cfg.bbox_lo[2] = domain->boxlo[2] - cutghost - 2.0;
  cfg.bbox_hi[2] = domain->boxlo[2] + h[2] + cutghost + 2.0;
  const int idummy = 0;
  const double ddummy[3] = {0, 0, 0};
  const double xdummy[3] = {0, 0, 0};
  int rc = mdp_md_setup(ctx, &cfg, n ? atom->x[0] : xdummy, n ? atom->v[0] : xdummy, atom->type, atom->tag, atom->mass,
                        style_id == 1 ? map : nullptr, &idummy, ddummy, &idummy, &idummy);
  if (rc != MDP_OK) return rc;
  if (with_mask) { // (an empty brick still SETS a mask: NULL would withdraw it)
    rc = mdp_md_set_mask(ctx, n ? atom->mask : &idummy);
    if (rc != MDP_OK) return rc;
  }
  static_assert(sizeof(imageint) == sizeof(int), "the device carries LAMMPS' 32-bit image flags (LAMMPS_SMALLBIG / SMALLSMALL)");
  rc = mdp_md_set_image(ctx, n ? reinterpret_cast<const int *>(atom->image) : &idummy);
  if (rc != MDP_OK) return rc;
  mdp_dd_config dd;
  memset(&dd, 0, sizeof dd);
  for (int d = 0; d < 3; d++) {
    dd.boxlo[d] = domain->boxlo[d];
    dd.procgrid[d] = comm->procgrid[d];
  }
  for (int k = 0; k < 6; k++) dd.h[k] = h[k];
  dd.rank = comm->me;
  dd.cutghost = cutghost;
  return mdp_dd_setup(ctx, &dd);
}

// the atoms the brick owns NOW, in the brick's order, into the host's arrays (x, v, tag, type, image; atom->nlocal follows).
// with_mask: atom->mask comes back with them (as mdp_brick_from_host sent it); without, the host has no group but `all`
// and every atom that comes back is in it
inline int mdp_brick_to_host(mdp_ctx *ctx, Atom *atom, bool with_mask)
{
  long long di[8];
  int rc = mdp_dd_info(ctx, di, nullptr, nullptr);
  if (rc != MDP_OK) return rc;
  const int n = (int) di[0];
  if (n + atom->nghost > atom->nmax) atom->avec->grow(n + atom->nghost); // (the host's idle passes over its stale ghosts stay inside)
  if (n) {
    if ((rc = mdp_md_download(ctx, atom->x[0], atom->v[0], nullptr, nullptr)) != MDP_OK) return rc;
    if ((rc = mdp_md_download_int(ctx, "tag", atom->tag)) != MDP_OK) return rc;
    if ((rc = mdp_md_download_int(ctx, "type", atom->type)) != MDP_OK) return rc;
    if ((rc = mdp_md_download_int(ctx, "image", reinterpret_cast<int *>(atom->image))) != MDP_OK) return rc;
    if (with_mask) {
      if ((rc = mdp_md_download_int(ctx, "mask", atom->mask)) != MDP_OK) return rc;
    } else
      for (int i = 0; i < n; i++) atom->mask[i] = 1;
  }
  atom->nlocal = n;
  return MDP_OK;
}

}    // namespace LAMMPS_NS

#endif
