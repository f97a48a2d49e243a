/* -*- c++ -*- -----------------------------------------------------------------------------------
   What the `fix heat/mdp` fixes of a run hand to the one `fix nve/mdp` (Fix::extract("mdp_heat_sources")): the number of
   heat/mdp fixes in Modify's list and, per fix in the order of that list, a copy of its settings and its group bit.  Every
   fix writes the count and its own slot in its init(), as the langevin/mdp fixes do (mdp_baths.h).
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_HEAT_H
#define MDP_HEAT_H

#include "mdpair_hip.h"

namespace LAMMPS_NS {

struct MdpHeatSources {
  int count;
  mdp_heat_config cfg[MDP_HEAT_MAXSRC];
  int bit[MDP_HEAT_MAXSRC];
};

}    // namespace LAMMPS_NS

#endif
