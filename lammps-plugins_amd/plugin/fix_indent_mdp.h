/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix indent/mdp`: LAMMPS `fix indent` on the device, for runs that integrate with `fix nve/mdp` on one MPI rank
   (host-linked or `bricks yes`), with or without `fix langevin/mdp` baths.  Not a time integrator: at init() it hands a
   copy of its settings to the one fix nve/mdp (its slot of Fix::extract "mdp_indenters", mdp_riders.h), which switches the
   library's indenters (mdp_indent_*, csrc/indent.hip) on in the context its steps run on for the length of each run.

   fix ID GROUP indent/mdp K sphere x y z R | cylinder dim c1 c2 R | plane dim pos lo|hi  [side in|out] [vel vx vy vz] units box

   LAMMPS' argument order.  The atoms of GROUP whose distance from the indenter's surface is dr < 0 feel K dr^2 out of its
   body; compute_scalar() is the indenter's energy sum -K/3 dr^3 and compute_vector(0..2) the force on it (thermo f_ID and
   f_ID[1..3]).  `vel` is this style's one extension: the centre moves at a constant velocity, as the LAMMPS deck
       variable x equal "vdisplace(x0, vx)" ...    fix ID GROUP indent K sphere v_x v_y v_z R units box
   does; a variable (v_name) is refused anywhere.  `units box` is required in words: LAMMPS' default, units lattice, is not
   supported.  Up to MDP_INDENT_MAX (4) of these fixes may stand next to one fix nve/mdp; they may share atoms.  Not next
   to fix nvt/mdp, fix heat/mdp or minimize/mdp, and not in a box with a non-periodic dimension (the device's minimum image
   wraps all three).  The mini-host has no fix_modify: the energy is read as f_ID.
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(indent/mdp,FixIndentMDP);
// clang-format on
#else

#ifndef MDP_FIX_INDENT_MDP_H
#define MDP_FIX_INDENT_MDP_H

#include "fix_rider_mdp.h"

namespace LAMMPS_NS {

class FixIndentMDP : public FixRiderMDP {
 public:
  FixIndentMDP(class LAMMPS *, int, char **);
  void init() override;
  double compute_scalar() override;
  double compute_vector(int) override;

 private:
  mdp_indent_config cfg;
  double last[MDP_INDENT_STATE_LEN] = {}; // energy and force of the last read (kept between runs), and the words behind them
  void periodic_or_refuse();     // refuses a box with a non-periodic dimension
  double number(const char *what, const char *s); // a finite number, or the refusal (a variable named as such)
};

}    // namespace LAMMPS_NS

#endif
#endif
