/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix setforce/mdp`, `fix addforce/mdp` and `fix aveforce/mdp`: LAMMPS `fix setforce`, `fix addforce` and `fix aveforce`
   with constant values on the device, for runs that integrate with `fix nve/mdp` on one MPI rank, with or without
   `fix langevin/mdp` baths, `fix indent/mdp` indenters and `fix spring/mdp` springs.  Not time integrators: at init() each
   hands a copy of its settings to the one fix nve/mdp (its slot of Fix::extract "mdp_gforces", mdp_riders.h), which switches
   the library's group forces (mdp_gforce_*, csrc/gforce.hip) on in the context its steps run on for the length of each run.

   fix ID GROUP setforce/mdp fx fy fz      (a number or NULL each; all NULL only measures)
   fix ID GROUP addforce/mdp fx fy fz      (numbers)
   fix ID GROUP aveforce/mdp fx fy fz      (a number or NULL each)

   LAMMPS' argument order.  compute_vector(0..2) is the total force on GROUP before the fix acted (thermo f_ID[1..3]), for
   all three styles; compute_scalar() the potential energy -f . sum xu of addforce (f_ID; 0 for the other two).  The three
   styles are one family: up to MDP_GFORCE_MAX (4) fixes of them may stand next to one fix nve/mdp, and they act on an
   atom's force in the order of their definition, as in LAMMPS -- with one restriction: a fix defined after an aveforce/mdp
   must not share atoms with it (the device walks an atom's fixes in one pass, and only an average needs the whole group
   first).  On the device the family runs behind fix indent/mdp and fix spring/mdp and in front of the Langevin force, so a
   setforce/mdp or aveforce/mdp is refused where LAMMPS' order would be another: an indent/mdp or spring/mdp defined after
   it, or a langevin/mdp defined before it, on shared atoms.  A variable (v_name), `region`, and addforce's `every` and
   `energy` are refused.  Not next to fix nvt/mdp, fix heat/mdp or minimize/mdp; addforce/mdp needs `bricks yes` (in the
   host-linked mode the host keeps atom->image), setforce/mdp and aveforce/mdp run in both modes.
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(setforce/mdp,FixSetForceMDP);
FixStyle(addforce/mdp,FixAddForceMDP);
FixStyle(aveforce/mdp,FixAveForceMDP);
// clang-format on
#else

#ifndef MDP_FIX_GFORCE_MDP_H
#define MDP_FIX_GFORCE_MDP_H

#include "fix_rider_mdp.h"

namespace LAMMPS_NS {

class FixGforceMDP : public FixRiderMDP {
 public:
  void init() override;
  double compute_scalar() override;
  double compute_vector(int) override;

 protected:
  FixGforceMDP(class LAMMPS *, int, char **, int kind, const char *name, const char *usage);

 private:
  mdp_gforce_config cfg;
  double last[MDP_GFORCE_STATE_LEN] = {};    // the words of the last read (kept between runs)
  double shared_with(const class Fix *other) const;    // atoms in this fix's group and in other's, over all ranks
};

class FixSetForceMDP : public FixGforceMDP {
 public:
  FixSetForceMDP(class LAMMPS *, int, char **);
};
class FixAddForceMDP : public FixGforceMDP {
 public:
  FixAddForceMDP(class LAMMPS *, int, char **);
};
class FixAveForceMDP : public FixGforceMDP {
 public:
  FixAveForceMDP(class LAMMPS *, int, char **);
};

}    // namespace LAMMPS_NS

#endif
#endif
