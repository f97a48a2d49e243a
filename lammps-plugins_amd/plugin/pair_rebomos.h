/* -*- c++ -*- -----------------------------------------------------------------------------------
   MI355X-native REBO Mo-S pair style: LAMMPS-facing adapter.

   Same class name, style name and virtual surface as the CPU plugin
   (lammps/lammps-plugins USER-REBOMOS/pair_rebomos.h:14-39) so that `pair_style rebomos` /
   `pair_coeff * * MoS.REBO.set5b Mo S` scripts run unchanged.  All arithmetic happens in
   libmdpair_hip.so (include/mdpair_hip.h); this class only moves the host's data across the C-ABI, and what it shares
   with the aeam adapter in doing so is its base class (pair_mdp.h).
-------------------------------------------------------------------------------------------------- */
#ifdef PAIR_CLASS
// clang-format off
PairStyle(rebomos,PairREBOMoS);
// clang-format on
#else

#ifndef MDP_PAIR_REBOMOS_H
#define MDP_PAIR_REBOMOS_H

#include "pair_mdp.h"

namespace LAMMPS_NS {

class PairREBOMoS : public PairMDP {
 public:
  PairREBOMoS(class LAMMPS *);
  void compute(int, int) override;
  void coeff(int, char **) override;
  void init_style() override;
  double init_one(int, int) override;
  double memory_usage() override;
  void *extract(const char *, int &) override;

 protected:
  bool host_list = false;       // MDP_REBOMOS_HOST_LIST=1: lists from the rows LAMMPS built (mdp_rebomos_host_list)
  mdp_rebomos_params params;    // the 61 file scalars after mixing
  bool params_read;
  double cut3rebo;              // 3 * rcmax_MM, the list cutoff the style asks the host for
  double device_bytes;
};

}    // namespace LAMMPS_NS

#endif
#endif
