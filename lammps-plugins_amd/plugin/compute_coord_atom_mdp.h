/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute coord/atom/mdp`: what compute coord/atom cutoff gives, for runs that fix nve/mdp (or fix nvt/mdp) keeps on the
   device in bricks mode.

   compute ID GROUP coord/atom/mdp cutoff Rc [jtype ...]        jtype = N, *, N*, *M or N*M

   A per-atom vector (no jtype, or one) or a per-atom array of one column per jtype (at most 32): for every owned atom of GROUP
   the number of atoms of ANY group, ghosts included, with rsq < Rc^2 and a type in the column's range; no jtype: all types.
   Atoms outside GROUP read 0.  Rc is at most the pair style's cutforce: what the brick's ghost shell guarantees between two
   reneighbourings.  LAMMPS' compute coord/atom reads the host's atom->x and neighbour list, which are stale while a brick run
   is under way; here the counts are formed on the device (mdp_coord_* through the run's context, compute_mdp.h) from the
   current positions.  The values are read on output steps -- thermo (through compute reduce), dump custom, the last step of a
   run -- when the atoms are home in the brick's order (compute_mdp.h, read_peratom).  Not supported, each refused with a
   message: the orientorder form, and the group keyword (the partners of a centre are the atoms of every group).  A context
   holds one measurement: two compute coord/atom/mdp in one input make each other send their setup again at every evaluation
   (a few words; the values stay right).
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(coord/atom/mdp,ComputeCoordAtomMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_COORD_ATOM_MDP_H
#define MDP_COMPUTE_COORD_ATOM_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeCoordAtomMDP : public ComputeMDP {
 public:
  ComputeCoordAtomMDP(class LAMMPS *, int, char **);
  ~ComputeCoordAtomMDP() override;
  void init() override;
  void compute_peratom() override;

 protected:
  double cutoff;
  std::vector<int> jlo, jhi;    // [ncol] inclusive type ranges
};

}    // namespace LAMMPS_NS

#endif
#endif
