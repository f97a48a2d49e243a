/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute msd/mdp`: LAMMPS' compute msd for runs that fix nve/mdp (or fix nvt/mdp) keeps on the device in bricks mode.

   compute ID GROUP msd/mdp [com yes|no] [average no]

   A global vector of 4: the mean over the group of dx^2, dy^2, dz^2 and their total, from the unwrapped positions
   x + h . image.  LAMMPS' own compute msd cannot serve a brick run: its origins are a host per-atom array, and the
   brick's atoms come back in another order, on other ranks.  Here the origins of ALL atoms are kept by tag (recorded at
   construction from the host's atom->x and atom->image, summed over the ranks) and uploaded once to the context the
   run's steps go through (compute_mdp.h); an evaluation is one pass over the brick's atoms on the device
   (mdp_msd_sums) and one sum over the ranks.  com yes: the displacement of the group's centre of mass is taken out.
   A context holds one measurement: a second compute msd/mdp in the same input makes both upload their origins again at
   every evaluation (24 bytes per atom each; the values stay right).
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(msd/mdp,ComputeMSDMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_MSD_MDP_H
#define MDP_COMPUTE_MSD_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeMSDMDP : public ComputeMDP {
 public:
  ComputeMSDMDP(class LAMMPS *, int, char **);
  ~ComputeMSDMDP() override;
  void init() override;
  void compute_vector() override;

 protected:
  int comflag;
  bigint nall;                 // atoms of the whole system: the origins are indexed by tag - 1
  std::vector<double> x0;      // [nall][3] unwrapped positions at construction, the same on every rank
  double cm0[3];               // the group's centre of mass there
  double out4[4];
};

}    // namespace LAMMPS_NS

#endif
#endif
