/* -*- c++ -*- -----------------------------------------------------------------------------------
   What the two MI355X pair adapters (pair_rebomos.h, pair_aeam.h) have in common: the device context and its choice of
   device, what `fix nve/mdp` reads and sets through Pair::extract, settings(), the argument checks and the setflag loop
   of coeff(), the upload stage of host-mode compute() and the whole of compute() while the fix keeps the atoms on its
   bricks.  The style's name and id are data members: pair_mdp.cpp is compiled into both plugin files and its symbols
   resolve to whichever file was loaded first, so its code must not depend on the style it was built next to.
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_PAIR_MDP_H
#define MDP_PAIR_MDP_H

#include "pair.h"

#include "mdpair_hip.h"

#include <string>

namespace LAMMPS_NS {

class PairMDP : public Pair {
 public:
  PairMDP(class LAMMPS *, const char *name, int style_id);
  ~PairMDP() override;
  void settings(int, char **) override;
  void *extract(const char *, int &) override;

 protected:
  const char *const name;       // "rebomos" / "aeam": the style's name in every message of this class
  int style_id;                 // MDP_STYLE_REBOMOS / MDP_STYLE_AEAM (what the fix sets its own context up with)
  bool overflow_is_neigh_one;   // fail_one() words MDP_EOVERFLOW as the reference does (pair_rebomos.cpp:350)
  mdp_ctx *dev;                 // device context (one GPU per rank)
  int nve_linked;               // set by fix nve/mdp: x, v and f of the owned atoms stay on the device between reneighborings
  int nve_mask;                 // set by fix nve/mdp on a group (or with a thermostat on one): atom->mask goes up with the velocities
  mdp_ctx *bricks;              // set by fix nve/mdp on several ranks: its context holds this rank's brick, whole steps run there
  int bricks_ev;                // ... and how it opened the current step: 1 energy / virial, 2 one brick, 4 per-atom tallies
  int nall_uploaded;            // atoms on the device match the host's (nlocal+nghost) of the last upload

  // what differs between the styles in the upload stage of compute()
  struct HostUpload {
    const double *box;          // domain->h where the library keeps the periodic images itself, else null
    const int *map;             // type -> element, or null
    bool host_rows;             // the lists are the host's rows (mdp_set_neighbors_host) ...
    int gnum;                   // ... with this many ghost rows; otherwise they come from the positions and the host's
    bool inum_is_nlocal;        //     list is only checked: (its row count first, ...
    int (*check)(mdp_ctx *, int, const int *, const int *, int *const *, double);
    double check_cut;           //     ... then) check(..., check_cut)
  };

  std::string prefix() const { return std::string("Pair style ") + name + " (MI355X)"; }
  void allocate();
  bool open_device();           // true when this call created the context
  void fail_one(int code, const char *what);
  void coeff_args(int narg, char **arg);
  void coeff_setflags(const double *element_mass = nullptr);
  bool linked() const;
  bool upload_host(const HostUpload &u);
  void compute_bricks();
};

}    // namespace LAMMPS_NS

#endif
