/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute cna/atom/mdp`: what compute cna/atom gives, for runs that fix nve/mdp (or fix nvt/mdp) keeps on the device in
   bricks mode.

   compute ID GROUP cna/atom/mdp Rc

   A per-atom vector: for every owned atom of GROUP the pattern of the common neighbour analysis of its neighbours (of any
   group, ghosts included) with rsq < Rc^2: 1 fcc, 2 hcp, 3 bcc, 4 icosahedral, 5 other; atoms outside GROUP read 0.  The
   signatures and the patterns are LAMMPS' (include/mdpair_hip.h, mdp_cna_read).  Two differences: the answer is formed from
   the current positions and not from a neighbour list of some age, and it does not depend on whether a neighbour is owned or
   a ghost, so Rc <= the pair style's cutforce suffices where LAMMPS asks 2 Rc <= cutforce + skin.  An atom with more than
   16 neighbours is `other`, as in LAMMPS, and a read that saw such atoms prints LAMMPS' warning, "Too many neighbors in CNA
   for N atoms", on the rank that saw them.
   The one extension, the census: a global vector of size 5, c_ID[1 .. 5] = the atoms of GROUP that are fcc, hcp, bcc,
   icosahedral, other, counted on the device and summed exactly over the ranks -- a thermo column, or the input of fix
   ave/time.  The values are formed on the device (mdp_cna_* through the run's context, compute_mdp.h) and read once per
   step, whichever of the per-atom vector and the census is asked for first; on output steps, when the atoms are home in the
   brick's order (compute_mdp.h, read_peratom).  A context holds one measurement: two compute cna/atom/mdp in one input make
   each other send their setup again at every evaluation.
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(cna/atom/mdp,ComputeCnaAtomMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_CNA_ATOM_MDP_H
#define MDP_COMPUTE_CNA_ATOM_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeCnaAtomMDP : public ComputeMDP {
 public:
  ComputeCnaAtomMDP(class LAMMPS *, int, char **);
  ~ComputeCnaAtomMDP() override;
  void init() override;
  void compute_peratom() override;
  void compute_vector() override;

 protected:
  double cutoff;
  double census[5];    // fcc, hcp, bcc, icosahedral, other: over all ranks, as of the last read
};

}    // namespace LAMMPS_NS

#endif
#endif
