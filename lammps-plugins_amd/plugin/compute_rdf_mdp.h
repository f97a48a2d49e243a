/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute rdf/mdp`: LAMMPS' compute rdf for runs that fix nve/mdp (or fix nvt/mdp) keeps on the device in bricks mode.

   compute ID GROUP rdf/mdp Nbin [itype1 jtype1 itype2 jtype2 ...] [cutoff Rc]

   A global array of Nbin rows and 1 + 2 npairs columns: the bin centre, then g(r) and the coordination number of every
   type pair, as compute rdf lays them out (a type argument is N, *, N*, *M or N*M; without pairs one column pair of all
   types with all types).  LAMMPS' own compute rdf cannot serve a brick run: it walks a host neighbour list of host
   positions, and the host's atom->x is stale while the run is under way.  Here the pairs are counted on the device from
   the brick's current atoms and ghosts (mdp_rdf_counts through the run's context, compute_mdp.h) in integers, summed
   exactly over the ranks, and normalised with the box of the current step.  The default cutoff, and the largest one, is the pair style's
   cutforce: the ghost shell is cutforce + skin wide as of the last reneighbouring.  Membership of the group is taken at
   init(), by tag.  A context holds one measurement: two compute rdf/mdp in one input make each other send their setup
   again at every evaluation (a few hundred bytes and the member table; the values stay right).
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(rdf/mdp,ComputeRDFMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_RDF_MDP_H
#define MDP_COMPUTE_RDF_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeRDFMDP : public ComputeMDP {
 public:
  ComputeRDFMDP(class LAMMPS *, int, char **);
  ~ComputeRDFMDP() override;
  void init() override;
  void compute_array() override;

 protected:
  int nbin, npairs, cutflag;
  double cutoff_user, cutoff;           // cutoff: the one in force (init())
  std::vector<int> ilo, ihi, jlo, jhi;  // [npairs] inclusive type ranges
  std::vector<unsigned char> member;    // [natoms] membership by tag - 1, the same on every rank; empty for group all
};

}    // namespace LAMMPS_NS

#endif
#endif
