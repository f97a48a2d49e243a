/* -*- c++ -*- -----------------------------------------------------------------------------------
   `minimize/mdp`: a FIRE minimisation (LAMMPS min_style fire with its defaults) that runs on the device from the first
   force to the last -- forces, sums, decisions, reneighbourings (csrc/fire.hip, mdp_fire_*).  A command style:

     minimize/mdp etol ftol maxiter maxeval [dmax d] [tmax t] [tmin t] [delaystep n] [dtgrow g] [dtshrink s]
                  [alpha0 a] [alphashrink a] [halfstepback yes|no] [initialdelay yes|no] [group ID]

   group ID: only the atoms of that group move; the others are held where they are, with the velocities they have, and
   stay out of the minimiser's sums and its force norm (what LAMMPS gives with fix setforce 0 0 0 on them).

   It does around a minimisation what `fix nve/mdp bricks yes` does around a run (plugin/mdp_brick.h): the host's atoms
   become one brick on a context of the command's own, on the pair style's device, with the style's parameters
   (Pair::extract); afterwards x, v, type, tag and mask come back in the brick's order, update->ntimestep has advanced by the
   iterations and update->dt is what it was.  One MPI rank, periodic box, atom_style atomic; fixes are not applied
   (INTEGRATION.md).
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
  int igroup = 0; // `group ID`: the atoms that move (0: all)
  void parse(int, char **);
  void fail(const char *what);
};

}    // namespace LAMMPS_NS

#endif
#endif
