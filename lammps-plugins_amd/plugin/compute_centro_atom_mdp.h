/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute centro/atom/mdp`: what compute centro/atom gives without its axes keyword, for runs that fix nve/mdp (or fix
   nvt/mdp) keeps on the device in bricks mode.

   compute ID GROUP centro/atom/mdp fcc|bcc|N [cutoff Rc]        fcc = 12, bcc = 8, N even and 2 .. 64

   A per-atom vector: for every owned atom of GROUP the N nearest atoms (of any group, ghosts included) among those with
   rsq < Rc^2, the N (N - 1) / 2 values |R_a + R_b|^2 of their pairs, and the sum of the N / 2 smallest.  An atom with fewer
   than N atoms inside Rc reads 0, as in LAMMPS; atoms outside GROUP read 0.  cutoff is the one extension: LAMMPS takes the N
   nearest of whatever its neighbour list holds, which depends on the list's age; here the answer depends on the state alone.
   The default Rc is the pair style's cutforce, the most the brick's ghost shell guarantees.  A centre with more than 128 atoms
   inside Rc refuses the read -- no centre is ever truncated --, and the message names cutoff: MoS2 at the default does this,
   the alloy at its 6.5 A (78 inside) does not.  The values are formed on the device (mdp_centro_* through the run's context,
   compute_mdp.h) and read on output steps, when the atoms are home in the brick's order (compute_mdp.h, read_peratom).
   Refused with a message: the axes keyword, an odd N, an N outside 2 .. 64.  A context holds one measurement: two compute
   centro/atom/mdp in one input make each other send their setup again at every evaluation.
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(centro/atom/mdp,ComputeCentroAtomMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_CENTRO_ATOM_MDP_H
#define MDP_COMPUTE_CENTRO_ATOM_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeCentroAtomMDP : public ComputeMDP {
 public:
  ComputeCentroAtomMDP(class LAMMPS *, int, char **);
  ~ComputeCentroAtomMDP() override;
  void init() override;
  void compute_peratom() override;

 protected:
  int nnn;
  double cutoff;    // 0: the pair style's cutforce (init())
};

}    // namespace LAMMPS_NS

#endif
#endif
