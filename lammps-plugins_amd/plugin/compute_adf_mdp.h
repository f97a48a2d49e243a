/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute adf/mdp`: LAMMPS' compute adf for runs that fix nve/mdp (or fix nvt/mdp) keeps on the device in bricks mode.

   compute ID GROUP adf/mdp Nbin [itype jtype ktype Rjinner Rjouter Rkinner Rkouter ...]
                                 [ordinate degree|radian|cosine] [cumulative fraction|centre]

   A global array of Nbin rows and 1 + 2 Ntriple columns: the bin centre of the ordinate, then per triple the angular
   distribution hist / (count delta) -- it integrates to 1 -- and its running sum, as compute adf lays them out (a type
   argument is N, *, N*, *M or N*M; without triples one triple * * * with both shells 0 .. cutforce).  `cumulative
   centre` divides the running sum by the number of central atoms and not by the number of angles: angles per centre, the
   angular coordination (the one extension).  LAMMPS' own compute adf cannot serve a brick run, for the reason given in
   compute_rdf_mdp.h.  Here the angles are counted on the device from the brick's current atoms and ghosts
   (mdp_adf_counts through the run's context, compute_mdp.h) in integers, summed exactly over the ranks.  The largest
   outer radius is the pair style's cutforce.  Membership of the group is taken at init(), by tag.  A context holds one
   adf measurement (next to its one rdf measurement): two compute adf/mdp in one input make each other send their setup
   again at every evaluation; the values stay right.
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(adf/mdp,ComputeADFMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_ADF_MDP_H
#define MDP_COMPUTE_ADF_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeADFMDP : public ComputeMDP {
 public:
  ComputeADFMDP(class LAMMPS *, int, char **);
  ~ComputeADFMDP() override;
  void init() override;
  void compute_array() override;

 protected:
  int nbin, ntriples, ordinate, per_centre;    // ordinate: MDP_ADF_DEGREE / _RADIAN / _COSINE; per_centre: cumulative centre
  bool default_shells;                         // no triple given: both shells 0 .. cutforce (init())
  std::vector<int> ilo, ihi, jlo, jhi, klo, khi;        // [ntriples] inclusive type ranges
  std::vector<double> rjin, rjout, rkin, rkout;         // [ntriples] shells
  std::vector<unsigned char> member;           // [natoms] membership by tag - 1, the same on every rank; empty for group all
};

}    // namespace LAMMPS_NS

#endif
#endif
