/* -*- c++ -*- -----------------------------------------------------------------------------------
   What the `fix spring/mdp` fixes of a run hand to the one `fix nve/mdp` (Fix::extract("mdp_springs")): the number of
   spring/mdp fixes in Modify's list and, per fix in the order of that list, a copy of its settings and its group bit (0:
   group all).  Every fix writes the count and its own slot in its init(), as the indent/mdp fixes do (mdp_indent.h).
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_SPRING_H
#define MDP_SPRING_H

#include "mdpair_hip.h"

namespace LAMMPS_NS {

struct MdpSprings {
  int count;
  mdp_spring_config cfg[MDP_SPRING_MAX];
  int bit[MDP_SPRING_MAX];
};

}    // namespace LAMMPS_NS

#endif
