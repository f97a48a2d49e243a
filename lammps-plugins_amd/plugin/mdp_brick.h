/* -*- c++ -*- -----------------------------------------------------------------------------------
   The host's atoms as one brick of the library's own decomposition and back: what `fix nve/mdp bricks yes` does around a
   run and `minimize/mdp` around a minimisation.  Free functions over the host's objects, so that a Fix and a Command
   (whose Pointers members are protected) share them.
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_BRICK_H
#define MDP_BRICK_H

#include "atom.h"
#include "atom_vec.h"
#include "comm.h"
#include "domain.h"
#include "force.h"
#include "neighbor.h"
#include "pair.h"
#include "update.h"

#include "mdpair_hip.h"

#include <cmath>
#include <cstring>

namespace LAMMPS_NS {

// this rank's owned atoms (x, v, type, tag as the host holds them) -> the brick of rank comm->me on comm->procgrid:
// mdp_md_setup + mdp_dd_setup.  style_id: 1 rebomos (map: the style's type -> element map), 2 aeam.  Returns the
// library's code; the message is mdp_last_error(ctx).
inline int mdp_brick_from_host(mdp_ctx *ctx, int style_id, const int *map, Atom *atom, Domain *domain, Force *force,
                               Neighbor *neighbor, Update *update, Comm *comm)
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

// the atoms the brick owns NOW, in the brick's order, into the host's arrays (x, v, tag, type; atom->nlocal follows)
inline int mdp_brick_to_host(mdp_ctx *ctx, Atom *atom)
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
  }
  atom->nlocal = n;
  return MDP_OK;
}

}    // namespace LAMMPS_NS

#endif
