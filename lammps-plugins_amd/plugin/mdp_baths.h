/* -*- c++ -*- -----------------------------------------------------------------------------------
   What the `fix langevin/mdp` fixes of a run hand to the one `fix nve/mdp` (Fix::extract("mdp_langevin_baths")): the
   number of langevin/mdp fixes in Modify's list and, per fix in the order of that list, a copy of its settings and its
   group bit.  Every fix writes the count and its own slot in its init(), so the hand-over does not depend on the order
   in which Modify calls the init()s.  bit 0 (one fix only): every atom the integrator moves.
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_BATHS_H
#define MDP_BATHS_H

#include "mdpair_hip.h"

namespace LAMMPS_NS {

struct MdpLangevinBaths {
  int count;
  mdp_langevin_config cfg[MDP_LANGEVIN_MAXBATH];
  int bit[MDP_LANGEVIN_MAXBATH];
};

}    // namespace LAMMPS_NS

#endif
