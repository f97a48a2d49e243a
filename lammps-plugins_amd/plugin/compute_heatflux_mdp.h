/* -*- c++ -*- -----------------------------------------------------------------------------------
   `compute heatflux/mdp`: LAMMPS' compute heat/flux (fed ke/atom, pe/atom and stress/atom NULL virial) for runs that
   fix nve/mdp (or fix nvt/mdp) keeps on the device in bricks mode.

   compute ID GROUP heatflux/mdp

   A global vector of 6, extensive (energy * velocity units, not divided by the volume, as compute heat/flux):
   J = sum (ke_i + pe_i) v_i + sum W_i . v_i in x, y, z, then its convective part sum (ke_i + pe_i) v_i in x, y, z.
   LAMMPS' own compute cannot serve a brick run: the per-atom computes it reads are host arrays, and the brick's atoms,
   energies and virials are on the device.  Here the compute asks for per-atom tallies on the steps it is due
   (peatomflag, pressatomflag, timeflag: Integrate::ev_set gives those steps the per-atom bits, fix nve/mdp opens them that
   way on the brick), and an evaluation is one pass over the brick's atoms on the device (mdp_heatflux_sums) and one sum
   over the ranks.  pe_i and W_i follow the reference's tally split (v_tally2/3, ev_tally3), not the centroid form.
-------------------------------------------------------------------------------------------------- */
#ifdef COMPUTE_CLASS
// clang-format off
ComputeStyle(heatflux/mdp,ComputeHeatFluxMDP);
// clang-format on
#else

#ifndef MDP_COMPUTE_HEATFLUX_MDP_H
#define MDP_COMPUTE_HEATFLUX_MDP_H

#include "compute_mdp.h"

namespace LAMMPS_NS {

class ComputeHeatFluxMDP : public ComputeMDP {
 public:
  ComputeHeatFluxMDP(class LAMMPS *, int, char **);
  ~ComputeHeatFluxMDP() override;
  void init() override;
  void compute_vector() override;

 protected:
  double out6[6];
};

}    // namespace LAMMPS_NS

#endif
#endif
