/* -*- c++ -*- -----------------------------------------------------------------------------------
   `minimize/mdp`: a FIRE minimisation (LAMMPS min_style fire with its defaults) that runs on the device from the first
   force to the last -- forces, sums, decisions, reneighbourings (csrc/fire.hip, mdp_fire_*).  A command style:

     minimize/mdp etol ftol maxiter maxeval [dmax d] [tmax t] [tmin t] [delaystep n] [dtgrow g] [dtshrink s]
                  [alpha0 a] [alphashrink a] [halfstepback yes|no] [initialdelay yes|no]

   It does around a minimisation what `fix nve/mdp bricks yes` does around a run (plugin/mdp_brick.h): the host's atoms
   become one brick on a context of the command's own, on the pair style's device, with the style's parameters
   (Pair::extract); afterwards x, v, type and tag come back in the brick's order, update->ntimestep has advanced by the
   iterations and update->dt is what it was.  One MPI rank, periodic box, group all, atom_style atomic; fixes are not
   applied.
-------------------------------------------------------------------------------------------------- */
#ifdef COMMAND_CLASS
// clang-format off
CommandStyle(minimize/mdp,MinimizeMDP);
// clang-format on
#else

#ifndef MDP_COMMAND_MINIMIZE_MDP_H
#define MDP_COMMAND_MINIMIZE_MDP_H

#include "command.h"

#include "mdpair_hip.h"

namespace LAMMPS_NS {

class MinimizeMDP : public Command {
 public:
  MinimizeMDP(class LAMMPS *lmp) : Command(lmp), ctx(nullptr) {}
  ~MinimizeMDP() override;
  void command(int, char **) override;

 private:
  mdp_ctx *ctx;
  mdp_fire_config cfg;
  void parse(int, char **);
  void fail(const char *what);
};

}    // namespace LAMMPS_NS

#endif
#endif
