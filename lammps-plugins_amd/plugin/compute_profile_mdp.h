/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute profile/mdp`: what compute chunk/atom bin/1d|2d|3d with fix ave/chunk, compute temp/chunk and compute vcm/chunk
   give, for runs that fix nve/mdp (or fix nvt/mdp) keeps on the device in bricks mode.

   compute ID GROUP profile/mdp dim N [dim N [dim N]] [com yes|no]        dim = x | y | z, all different

   A global array of N1 [N2 [N3]] rows (the first named dimension slowest) and ndim + 7 columns: the bin centre in each named
   dimension in reduced units (b + 0.5) / N; count; density/number = count / Vbin; density/mass = mv2d sum(m) / Vbin; temp;
   vcm x, y, z = sum(m v) / sum(m), the bin's centre-of-mass velocity as compute vcm/chunk gives it.  Vbin = the box volume
   of the current step / rows.  temp = mvv2e K / (3 count boltz) with K = sum(m v^2) (com no, the default) or
   sum(m v^2) - |sum(m v)|^2 / sum(m) (com yes: about the bin's own flow).  An empty bin reads 0 in every value column.
   The bins span the box in reduced units, triclinic included; a periodic dimension wraps, a non-periodic one counts an
   atom beyond the box in its edge bin.  LAMMPS' own chunk computes read the host's atom->x and atom->v, which are stale
   while a brick run is under way.  Here the sums are formed on the device (mdp_profile_* through
   the run's context, compute_mdp.h) as 64-bit integers with one power-of-two scale per column that every rank derives from the
   global range: the table does not depend on the decomposition.  Membership of the group goes with the atoms (atom->mask
   on the device).  A context holds one measurement: two compute profile/mdp in one input make each other send their bins
   again at every evaluation (a few words; the values stay right).
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(profile/mdp,ComputeProfileMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_PROFILE_MDP_H
#define MDP_COMPUTE_PROFILE_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeProfileMDP : public ComputeMDP {
 public:
  ComputeProfileMDP(class LAMMPS *, int, char **);
  ~ComputeProfileMDP() override;
  void init() override;
  void compute_array() override;

 protected:
  int ndim, comflag;
  int dim[3], nbin[3];                  // the named dimensions in the order given, and their bins
  long long nrows;                      // the array is [nrows][ndim + 7]
};

}    // namespace LAMMPS_NS

#endif
#endif
