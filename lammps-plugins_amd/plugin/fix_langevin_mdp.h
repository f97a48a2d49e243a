/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix langevin/mdp`: LAMMPS `fix langevin` on the device, for runs that integrate with `fix nve/mdp` (any of its modes:
   host-linked, `bricks yes`, several ranks).  Not a time integrator: at init() it hands a copy of its settings to the
   one fix nve/mdp (its slot of Fix::extract "mdp_langevin_baths", mdp_riders.h), which switches the library's thermostat
   (mdp_langevin_*, csrc/langevin.hip) on in the context its steps run on for the length of each run.

   Up to MDP_LANGEVIN_MAXBATH (4) of these fixes may stand next to one fix nve/mdp -- a hot and a cold bath, say -- if no
   atom is in the groups of two of them (LAMMPS would add both forces on such an atom; init() refuses it and names both
   fixes and the number of atoms).  Each then is a bath of its own: its numbers, its `zero` mean over its group, and its
   tally, which its compute_scalar() returns (thermo f_ID; ecouple sums them).

   fix ID GROUP langevin/mdp Tstart Tstop damp seed [scale type ratio ...] [tally yes|no] [zero yes|no]

   GROUP: a group whose atoms fix nve/mdp integrates (its group or a part of it; all only next to fix ID all nve/mdp): the
   force, the mean `zero yes` takes out and the tally then run over that group alone.  No variables, gjf, angmom or omega; zero and tally on one MPI rank.  The noise is keyed by atom tag and
   step, not LAMMPS' per-rank stream.  compute_scalar() is the thermostat energy with tally yes
   (ecouple_flag = 1), 0 otherwise.
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(langevin/mdp,FixLangevinMDP);
// clang-format on
#else

#ifndef MDP_FIX_LANGEVIN_MDP_H
#define MDP_FIX_LANGEVIN_MDP_H

#include "fix_rider_mdp.h"

namespace LAMMPS_NS {

class FixLangevinMDP : public FixRiderMDP {
 public:
  FixLangevinMDP(class LAMMPS *, int, char **);
  void init() override;
  double compute_scalar() override;

 private:
  mdp_langevin_config cfg;
};

}    // namespace LAMMPS_NS

#endif
#endif
