/* -*- c++ -*- -----------------------------------------------------------------------------------
   What the `fix indent/mdp` fixes of a run hand to the one `fix nve/mdp` (Fix::extract("mdp_indenters")): the number of
   indent/mdp fixes in Modify's list and, per fix in the order of that list, a copy of its settings and its group bit (0:
   group all).  Every fix writes the count and its own slot in its init(), as the heat/mdp fixes do (mdp_heat.h).
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_INDENT_H
#define MDP_INDENT_H

#include "mdpair_hip.h"

namespace LAMMPS_NS {

struct MdpIndenters {
  int count;
  mdp_indent_config cfg[MDP_INDENT_MAX];
  int bit[MDP_INDENT_MAX];
};

}    // namespace LAMMPS_NS

#endif
