/* -*- c++ -*- -----------------------------------------------------------------------------------
   `fix nve/mdp`: velocity-Verlet NVE on the device, for runs whose pair style is one of this plugin's.

   The reference's styles run under the host's `fix nve` (in.rebomos-bulk:27): atom->f comes down and atom->x goes
   up across the link every step.  This fix does the two half-kicks and the drift on the device through the pair
   style's context (Pair::extract("mdp_ctx")), so that between two reneighborings nothing per atom crosses the link.
   A plugin registering a fix style is what the reference repository itself does (USER-BFIELD/bfieldplugin.cpp:15-29,
   creator.v2; virtuals USER-BFIELD/fix_bfield.h:33-38).

   fix ID GROUP nve/mdp [hostcheck yes|no] [bricks yes|no]     (defaults no, no: see fix_nve_mdp.cpp)

   GROUP: all, or any group of the group command.  The atoms outside it keep their positions and velocities bit for bit
   (LAMMPS' fix nve on a group): atom->mask goes to the device with the atoms, in every mode, and the integrate kernels
   honour the fix's group bit (mdp_integrate_group).  Group all runs exactly the kernels it always did.

   On several MPI ranks the fix runs the library's own domain decomposition (csrc/domain.hip: one brick per rank on
   Comm's processor grid, halo / migration / `check yes` decision on the device, RCCL between the GPUs) on a context of
   its own, from the atoms each rank owns at setup; the host's Comm and Neighbor idle for the length of the run and get
   the atoms back -- wherever they migrated to -- on output steps and at the end (fix_nve_mdp.cpp, "bricks").
-------------------------------------------------------------------------------------------------- */
#ifdef FIX_CLASS
// clang-format off
FixStyle(nve/mdp,FixNVEMDP);
// clang-format on
#else

#ifndef MDP_FIX_NVE_MDP_H
#define MDP_FIX_NVE_MDP_H

#include "fix.h"

#include "mdp_riders.h"
#include "mdpair_hip.h"

namespace LAMMPS_NS {

class FixNVEMDP : public Fix {
 public:
  FixNVEMDP(class LAMMPS *, int, char **);
  ~FixNVEMDP() override;
  int setmask() override;
  void init() override;
  void setup(int) override;
  void initial_integrate(int) override;
  void final_integrate() override;
  void post_run() override;
  void reset_dt() override;
  void *extract(const char *, int &) override;

 protected:
  mdp_ctx **ctxp;      // the pair style's device context (created in its init_style)
  int *pair_linked;    // the pair style's "positions and forces stay on the device" switch
  int *pair_mask;      // the pair style's "atom->mask goes up with the velocities" switch (a group, or a thermostat on one)
  long downloads;      // steps on which the host's x / v were brought up to date (statistics)
  int hostcheck;       // `hostcheck yes`: Neighbor::decide() keeps looking at atom->x, which is downloaded for it
  int took_delay;      // init() raised neighbor->delay (`check yes`: the device's check decides) ...
  int saved_delay;     // ... from this value, which the destructor restores
  static constexpr int kDelayTaken = 1 << 30;

  class Pair *linked_to; // the pair style ctxp / pair_linked / bricks_slot point into (see the destructor)
  // several ranks ("bricks")
  int bricks;          // comm->nprocs > 1, or `bricks yes`: the steps run on bctx
  int bricks_kw;       // `bricks yes`
  int bricks_want = 0; // what `bricks` will be once init() has run (extract "mdp_bricks_want": a fix whose init() runs first asks this)
  long one_rank_builds = 0;
  mdp_ctx *bctx;       // the fix's own context: this rank's brick
  mdp_ctx **bricks_slot;   // the pair style's pointer to it (set while a run is under way: its compute() ends the steps there)
  int *bricks_ev;      // the pair style's copy of "this step was opened with energy / virial"
  int style_id, comm_up, pending_final, step_ev;
  const int *bricks_map = nullptr; // rebomos: the pair style's type -> element map, as of the last init()
  // per-atom tally steps (compute heatflux/mdp): every compute that asks for per-atom energy or virial reads them on the
  // device (a /mdp style) -- then a step LAMMPS opens with VIRIAL_ATOM tallies eatom / vatom on the brick; a host
  // compute among them would read zeros, so the pair style stops such a step as it always has
  int atom_ok = 0;
  long atom_steps = 0; // computes with per-atom tallies in this run (MDP_FIX_STATS)
  static constexpr int kVirialAtom = 4; // VIRIAL_ATOM of LAMMPS' force.h: the bit of the vflag Integrate::ev_set hands out
  bool atom_step(int vflag) const { return atom_ok && (vflag & kVirialAtom); }

  // What the fixes that ride on this one handed over (fix_rider_mdp.h; one block per style, mdp_riders.h, under the
  // Fix::extract key beside it): switched on in setup() on run_ctx, behind the groups and the mask, in the order they
  // stand here -- heat sources (mdp_heat_setup, mdp_heat_run(beginstep)), indenters, behind them springs and behind those the
  // group forces (the order of the passes in front of a kick), Langevin thermostats (one: mdp_langevin_setup, mdp_langevin_group; several:
  // mdp_langevin_baths) -- and off in post_run(), which clears the blocks.  A style takes part in a run if its count > 0
  MdpHeatSources heat = {};      // "mdp_heat_sources"
  MdpIndenters indent = {};      // "mdp_indenters"
  MdpSprings spring = {};        // "mdp_springs": bricks only, the fixes refuse the host-linked mode
  MdpGforces gforce = {};        // "mdp_gforces": fix setforce/mdp, addforce/mdp and aveforce/mdp share its slots
  MdpLangevinBaths baths = {};   // "mdp_langevin_baths"
  // f(block, key, off, against, refusal) for each of them; against: the count of the kind it cannot share a run with, or null
  template <class F> void riders(F f)
  {
    f(heat, "mdp_heat_sources", mdp_heat_off, &baths.count, "Fix nve/mdp: heat sources (fix heat/mdp) and a thermostat (fix langevin/mdp) in one run");
    f(indent, "mdp_indenters", mdp_indent_off, &heat.count, "Fix nve/mdp: indenters (fix indent/mdp) and heat sources (fix heat/mdp) in one run");
    f(spring, "mdp_springs", mdp_spring_off, &heat.count, "Fix nve/mdp: springs (fix spring/mdp) and heat sources (fix heat/mdp) in one run");
    f(gforce, "mdp_gforces", mdp_gforce_off, &heat.count,
      "Fix nve/mdp: group forces (fix setforce/mdp, addforce/mdp, aveforce/mdp) and heat sources (fix heat/mdp) in one run");
    f(baths, "mdp_langevin_baths", mdp_langevin_off, (const int *) nullptr, "");
  }
  int brick_masked = 0; // this run's brick was set up with atom->mask (it comes back with the atoms)
  // the context the steps of the run under way go through, null between runs (extract "mdp_steps_ctx": the computes read
  // their sums there and the riding fixes their state); extract "mdp_bricks": whether that context is a brick of the library's own
  mdp_ctx *run_ctx = nullptr;

  mdp_ctx *ctx() const { return ctxp ? *ctxp : nullptr; }
  void setup_steps(int vflag);
  void to_host(bool forces);
  void init_bricks();
  void bricks_to_host();
  void fail(mdp_ctx *c);
  int taken_delay() const;
  bool grouped() const { return igroup > 0; }                  // the fix acts on a group other than all
  bool masked();                                               // ... or a fix that rides on this one does: the device needs atom->mask
  bool brick_mask();                                           // bricks: atom->mask travels with the atoms
  double group_count();                                        // atoms the fix integrates, over all ranks
  void apply_groups(mdp_ctx *c);                               // the group bits (and, host-linked, the mask) of this run on c
};

}    // namespace LAMMPS_NS

#endif
#endif
