/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix spring/mdp`: LAMMPS `fix spring tether` on the device, for runs that integrate with `fix nve/mdp bricks yes` on one
   MPI rank, with or without `fix langevin/mdp` baths and `fix indent/mdp` indenters.  Not a time integrator: at init() it
   hands a copy of its settings to the one fix nve/mdp (its slot of Fix::extract "mdp_springs", mdp_riders.h), which switches
   the library's springs (mdp_spring_*, csrc/spring.hip) on in the context its steps run on for the length of each run.

   fix ID GROUP spring/mdp tether K x y z R0 [vel vx vy vz]

   LAMMPS' argument order.  A spring of stiffness K and rest length R0 between the centre of mass of GROUP, taken over the
   unwrapped positions, and the tether point (x, y, z); each of x, y, z may be NULL, and that dimension then takes no part.
   compute_scalar() is the spring's energy K (r - R0)^2 / 2 and compute_vector(0..3) the force on the group and its signed
   magnitude (thermo f_ID and f_ID[1..4]).  `vel` is this style's one extension, as on fix indent/mdp: the tether point moves
   at a constant velocity (the constant-velocity mode of fix smd); a variable (v_name) is refused anywhere, and so is
   `couple`.  Up to MDP_SPRING_MAX (4) of these fixes may stand next to one fix nve/mdp; they may share atoms.  Not next to
   fix nvt/mdp, fix heat/mdp or minimize/mdp, and not in the host-linked mode, where the host keeps atom->image.
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(spring/mdp,FixSpringMDP);
// clang-format on
#else

#ifndef MDP_FIX_SPRING_MDP_H
#define MDP_FIX_SPRING_MDP_H

#include "fix_rider_mdp.h"

namespace LAMMPS_NS {

class FixSpringMDP : public FixRiderMDP {
 public:
  FixSpringMDP(class LAMMPS *, int, char **);
  void init() override;
  double compute_scalar() override;
  double compute_vector(int) override;

 private:
  mdp_spring_config cfg;
  double last[MDP_SPRING_STATE_LEN] = {}; // energy and ftotal of the last read (kept between runs), and the words behind them
  double number(const char *what, const char *s); // a finite number, or the refusal (a variable named as such)
};

}    // namespace LAMMPS_NS

#endif
#endif
