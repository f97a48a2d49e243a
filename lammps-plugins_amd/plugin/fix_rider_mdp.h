/* -*- c++ -*- -----------------------------------------------------------------------------------
   FixRiderMDP: what the fixes that ride on `fix nve/mdp` share -- fix langevin/mdp, fix heat/mdp, fix indent/mdp, fix
   spring/mdp and the family fix setforce/mdp, addforce/mdp, aveforce/mdp.  None of them integrates: each hands a copy of its settings to the one fix nve/mdp of a run (its slot of the
   block of its style, mdp_riders.h), which switches the library feature on in its setup() and off in its post_run().  Not a
   style: compiled into each rider's plugin file, and it reaches fix nve/mdp through Fix::extract alone.

     constructor      the style's usage for too few arguments, then the two group refusals (unknown, empty)
     setmask          0: the work runs inside fix nve/mdp's device steps
     integrator       the fix nve/mdp of this run (looked up anew: no pointer outlives either fix)
     census           the fixes of this style in Modify's list and this fix's slot among them; refuses one too many.  A fix
                      with this fix's ID does not count: this one is replacing it.  A style may belong to a family of style
                      names that share one block of slots (kin): then the fixes of all of them count, in Modify's order
     inside           refuses a group with an atom the integrator does not move
     disjoint         refuses atoms shared with a fix of this style earlier in Modify's list
     walk             from init(): Modify's list once -- the integrator, the slot and the count; refuses the styles this one
                      cannot stand next to, a host-side integrator and a run without fix nve/mdp
     handover         the style's block of that fix nve/mdp, or the refusal
     populated        the empty-group refusal again, for a group that lost its atoms since
     read             this fix's state words from the context of the run under way; between runs nothing is read
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_FIX_RIDER_MDP_H
#define MDP_FIX_RIDER_MDP_H

#include "fix.h"

#include "mdp_riders.h"

#include <initializer_list>
#include <string>
#include <vector>

namespace LAMMPS_NS {

class FixRiderMDP : public Fix {
 public:
  int setmask() override { return 0; }

 protected:
  // name: "heat/mdp"; max: how many of them fix nve/mdp takes; key: the Fix::extract key of their block; usage: said for
  // fewer than min_narg arguments; empty_tail: what an empty group leaves out, "there is no atom to heat"; family: the
  // style names that share the block with `name` (itself among them), none for a style with a block of its own
  FixRiderMDP(class LAMMPS *, int, char **, const char *name, int max, const char *key, int min_narg, const char *usage,
              const char *empty_tail, std::initializer_list<const char *> family = {});

  const std::string name;
  int slot = 0;    // this fix's position among the fixes of its style in Modify's list, as of the last init()
  typedef int (*state_fn)(mdp_ctx *, int, double *);

  class Fix *integrator() const;
  bool kin(const char *style) const;    // a style of this fix's family (its own, without one)
  int census();
  void inside(class Fix *nve, const char *noun);    // noun: "source", in "the source acts on atoms the integrator moves"
  void disjoint();
  // refused: the styles this one cannot stand next to, said as "Fix <name>: fix " + before + ID + " (style" + after;
  // host: behind "integrates on the host; "; lacking: the whole sentence of a run without fix nve/mdp
  class Fix *walk(std::initializer_list<const char *> refused, const std::string &before, const char *after, const char *host,
                  const char *lacking, int &count);
  void *handover(class Fix *nve, const char *takes); // takes: "heat sources", in "does not take heat sources"
  double populated();                                // the atoms of the group over all ranks; refuses none
  // out = fn(slot) of the run under way, false between runs.  once: one blocking read per step serves f_ID and f_ID[k]
  bool read(state_fn fn, double *out, bool once = false);

 private:
  const int max;
  const char *const key, *const empty_tail;
  std::vector<std::string> family;    // empty: the style stands alone
  std::string kind() const;           // how a message names the fixes that are counted: the style, or the family's styles
  bigint read_step = -1;    // the timestep a `once` read was last made at in this run (-1: not yet)
};

}    // namespace LAMMPS_NS

#endif
