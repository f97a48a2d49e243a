/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix nvt/mdp`: LAMMPS `fix nvt` (Nose-Hoover chain, thermostat only) on the device, for runs whose pair style is one of
   this project's.  A subclass of `fix nve/mdp` in its one-rank modes (host-linked, and `bricks yes`): the same steps, with
   the library's thermostat (mdp_nhc_*, csrc/nhc.hip) switched on in the context the steps run on.

   fix ID GROUP nvt/mdp temp Tstart Tstop Tdamp [tchain M] [tloop L] [drag d] [hostcheck yes|no] [bricks yes|no]

   One MPI rank, no barostat.  GROUP: all, or any group of the group command -- the chain then thermostats that group
   (its kinetic energy, 3 N_group - 3 degrees of freedom, its velocities) and the other atoms keep x and v (fix_nve_mdp.h).  compute_scalar() is the thermostat energy (ecouple_flag = 1); the chain persists
   across `run` commands (read back in post_run, seeded again in setup).
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(nvt/mdp,FixNVTMDP);
// clang-format on
#else

#ifndef MDP_FIX_NVT_MDP_H
#define MDP_FIX_NVT_MDP_H

#include "fix_nve_mdp.h"

#include <vector>

namespace LAMMPS_NS {

class FixNVTMDP : public FixNVEMDP {
 public:
  FixNVTMDP(class LAMMPS *, int, char **);
  void init() override;
  void setup(int) override;
  void post_run() override;
  double compute_scalar() override;

 private:
  struct Args {
    std::vector<char *> nve; // what fix nve/mdp parses: ID group style [hostcheck ..] [bricks ..]
    mdp_nhc_config cfg;
  };
  static Args parse(class LAMMPS *, int, char **);
  FixNVTMDP(class LAMMPS *, Args);

  mdp_nhc_config ncfg;
  double chain[MDP_NHC_STATE_LEN]; // the chain between runs (mdp_nhc_state layout)
  int have_chain;
  mdp_ctx *nhc_ctx;                // the context the thermostat was set up on for the current run
  bigint run_first, run_last;      // the ramp of the current run

  void nhc_fail(mdp_ctx *c);
};

}    // namespace LAMMPS_NS

#endif
#endif
