/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix heat/mdp`: LAMMPS `fix heat` with a constant flux on the device, for runs that integrate with `fix nve/mdp` on one
   MPI rank (host-linked or `bricks yes`).  Not a time integrator: at init() it hands a copy of its settings to the one
   fix nve/mdp (its slot of Fix::extract "mdp_heat_sources", mdp_riders.h), which switches the library's heat sources
   (mdp_heat_*, csrc/heat.hip) on in the context its steps run on for the length of each run.

   fix ID GROUP heat/mdp N eflux

   Every N steps the atoms of GROUP gain eflux N dt of kinetic energy about their centre of mass (eflux in energy / time,
   negative: a sink) and keep their momentum -- FixHeat::end_of_step, behind the final half of the step on the device.  Up
   to MDP_HEAT_MAXSRC (4) of these fixes may stand next to one fix nve/mdp -- a source and a sink, say -- if no atom is in
   the groups of two of them.  GROUP: atoms fix nve/mdp integrates.  No variable flux, no region; no thermostat (fix
   nvt/mdp, fix langevin/mdp) in the same run.  compute_scalar() is the factor the velocities about the centre of mass were
   scaled by at the last application (thermo f_ID), as FixHeat's.
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(heat/mdp,FixHeatMDP);
// clang-format on
#else

#ifndef MDP_FIX_HEAT_MDP_H
#define MDP_FIX_HEAT_MDP_H

#include "fix_rider_mdp.h"

namespace LAMMPS_NS {

class FixHeatMDP : public FixRiderMDP {
 public:
  FixHeatMDP(class LAMMPS *, int, char **);
  void init() override;
  double compute_scalar() override;

 private:
  mdp_heat_config cfg;
  double scale = 1.0;            // of the last application read (kept between runs, as FixHeat keeps it)
};

}    // namespace LAMMPS_NS

#endif
#endif
