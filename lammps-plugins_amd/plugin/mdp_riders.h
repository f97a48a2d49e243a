/* -*- c++ -*- -----------------------------------------------------------------------------------
   What the fixes of one style that ride on `fix nve/mdp` (fix_rider_mdp.h) hand to it, through Fix::extract under the
   style's key: the number of these fixes in Modify's list and, per fix in the order of that list, a copy of its settings
   and its group bit (0: every atom the integrator moves, no mask needed for this fix's sake).  A family of styles may share
   one block (fix setforce/mdp, addforce/mdp and aveforce/mdp: "mdp_gforces"): its slots are the family's fixes in that order.  Every fix writes the count
   and its own slot in its init(), so the hand-over does not depend on the order in which Modify calls the init()s.
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_RIDERS_H
#define MDP_RIDERS_H

#include "mdpair_hip.h"

namespace LAMMPS_NS {

template <typename Config, int MAX> struct MdpRiders {
  int count;
  Config cfg[MAX];
  int bit[MAX];

  bool masked() const    // some slot has a group bit: the device needs atom->mask
  {
    for (int k = 0; k < count; k++)
      if (bit[k]) return true;
    return false;
  }
};

typedef MdpRiders<mdp_langevin_config, MDP_LANGEVIN_MAXBATH> MdpLangevinBaths;    // "mdp_langevin_baths"
typedef MdpRiders<mdp_heat_config, MDP_HEAT_MAXSRC> MdpHeatSources;               // "mdp_heat_sources"
typedef MdpRiders<mdp_indent_config, MDP_INDENT_MAX> MdpIndenters;                // "mdp_indenters"
typedef MdpRiders<mdp_spring_config, MDP_SPRING_MAX> MdpSprings;                  // "mdp_springs"
typedef MdpRiders<mdp_gforce_config, MDP_GFORCE_MAX> MdpGforces;                  // "mdp_gforces"

}    // namespace LAMMPS_NS

#endif
