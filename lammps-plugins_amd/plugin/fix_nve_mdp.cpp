/* ------------------------------------------------------------------------------------------------
   fix nve/mdp -- see fix_nve_mdp.h.  What runs where:

     initial_integrate   v += dtf f/m, x += dt v, periodic images refreshed            device (mdp_hnve_initial)
     Pair::compute       no position upload, forces stay on the device               device
     final_integrate     v += dtf f/m                                                device (mdp_hnve_final)

   and the host's atom->x / atom->v are brought up to date only on steps where the host reads them:
     * a reneighboring: Neighbor::decide() is asked for one through force_reneighbor / next_reneighbor when the
       device's own displacement check (half the skin, read one step late, with a margin) fires.  That check IS
       `neigh_modify check yes` -- the same quantity Neighbor::check_distance() computes from atom->x, seen earlier (the
       margin) -- so under `check yes` (the default; in.rebomos-bulk runs with every 1 delay 0 check yes,
       log.rebomos-bulk.1:41, sample.in:18 with every 1 delay 1 check yes) the fix takes the host's own check out of the
       steps: init() raises neighbor->delay beyond any run and the destructor puts it back.  The inputs of the
       reference then run unchanged at the device's speed; the host's x would be stale for its check anyway.
       `fix ID all nve/mdp hostcheck yes` keeps the host's settings as they are instead and downloads x and v on every
       step on which decide() looks at atom->x (the behaviour of the first version: correct for every setting, one
       download per look).  Under `check no` decide() rebuilds by the calendar, and x / v come down for exactly those steps;
     * thermo / dump steps (output->next) and the last step of a run.
   On one MPI rank the pair style keeps the periodic images itself (mdp_set_box_host), so ghosts follow their owners
   without the host's forward_comm.

   `fix ID all nve/mdp bricks yes` on ONE rank runs the mode described next with a single brick (no communicator): the
   periodic images, the lists and every reneighboring are then the device's too (mdp_md_integrate_check, mdp_dd_reneighbor,
   mdp_md_compute) and the host's Neighbor idles for the length of the run -- 2.88 against 3.08 ms per step at 3.98 M atoms
   from rest, and for hot runs the difference between a reneighboring of 2 ms on the device and one on the host (sample.in's
   alloy at 1.0 M atoms: 1.12 ms per step).  Not the default on one rank: per-atom energy / virial for a compute on the host
   and a non-periodic box need the mode above.  (Per-atom tallies for a reader on the device -- compute heatflux/mdp -- are
   taken on the brick: a step LAMMPS opens with VIRIAL_ATOM runs with eflag | 2, vflag | 4 there when every compute that
   asks for per-atom tallies is a /mdp style, see init_bricks; bit 4 of the pair style's bricks_ev.)

   Several ranks ("bricks").  There the host's Comm owns ghosts and migration, on host arrays -- which is what this fix
   takes out of the steps.  So it runs the library's own decomposition instead, as minihost/ddhost.cpp does without a
   LAMMPS around it:
     init()              a context of its own (same device as the pair style's), the style's parameters / tables on it
                         (mdp_own_context, mdp_brick.h); neighbor->delay beyond any run: the host neither checks nor reneighbors
     setup()             this rank's owned atoms (x, v, type, tag as the host holds them after ITS setup) -> the brick
                         (mdp_md_setup, mdp_dd_setup on comm->procgrid, rank = comm->me: LAMMPS' own bricks); RCCL's id from
                         rank 0 with MPI_Bcast(world); first halo and lists (mdp_dd_comm_reneighbor); forces of step 0
     initial_integrate   mdp_dd_comm_step_begin: half-kick + drift, the `check yes` decision from the word that rode in the
                         previous halo, migration + lists or the start of this step's halo, what needs no remote ghost
     Pair::compute       mdp_dd_comm_step_end (PairMDP::compute_bricks): the rest of the step; eng_vdwl / virial of
                         this rank's atoms on steps that ask (the host sums over ranks as it always does)
     final_integrate     output steps and the last step: atoms come back -- as many as the brick owns NOW (atom->nlocal
                         and, through atom->avec->grow, the arrays follow), x, v, type, tag
     post_run            the pair style is released: the next run starts from the host's arrays like the first
   What the host still does every step is idle work on stale arrays (Comm::forward_comm / reverse_comm of its ghosts, a
   memset of f); arrays never shrink below nlocal + the stale ghosts, so that work stays inside them.  atom->mask travels
   with the atoms whenever the host has a group besides all, and atom->image always does: the device's remap counts the
   box vectors it takes off an atom (mdp_md_set_image), so unwrapped coordinates and displacements are right after a
   bricks run, and compute msd/mdp reads them during one (Fix::extract("mdp_steps_ctx"), "mdp_bricks").  Per-atom
   properties beyond the atomic style's are not carried -- atom_style atomic.

   Groups (`fix ID GROUP nve/mdp`, GROUP other than all).  The fix's group bit goes to the library (mdp_integrate_group),
   and atom->mask with the atoms: next to the velocities at every host reneighboring in the host-linked mode
   (PairMDP::upload_host, mdp_hnve_set_mask), with the atoms into the brick otherwise (mdp_brick.h, mdp_md_set_mask),
   from where it comes back with them.  A fix langevin/mdp on a sub-group hands its bit over the same way
   (mdp_langevin_group), several of them on disjoint sub-groups their bits and settings together (mdp_langevin_baths), and
   the fix heat/mdp, fix indent/mdp, fix spring/mdp and fix setforce/mdp, addforce/mdp, aveforce/mdp fixes of a run theirs (mdp_heat_setup and its like, in setup() behind
   the mask).  Group all sets both bits to 0 and uploads no mask for the fix's sake.  All of these styles ride on this fix the
   same way (fix_rider_mdp.h): one block per style (mdp_riders.h) that they fill at init(), one list of the blocks
   (riders(), fix_nve_mdp.h) that setup(), post_run(), extract() and masked() walk, and one pointer, run_ctx, to the context
   of the run under way, which they and the computes read through Fix::extract("mdp_steps_ctx").  Run in the mini-host
   on 2, 4 and 8 ranks (tests/test_gpu_minilmp_ranks.py: log.rebomos-bulk.4's rows, the one-rank thermo of hot runs with
   migration); against a real LAMMPS this mode is unverified.
-------------------------------------------------------------------------------------------------- */
#include "fix_nve_mdp.h"
#include "mdp_brick.h"

#include "atom.h"
#include "atom_vec.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "compute.h"
#include "group.h"
#include "modify.h"
#include "neighbor.h"
#include "output.h"
#include "pair.h"
#include "update.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace LAMMPS_NS;
using namespace FixConst;

FixNVEMDP::FixNVEMDP(LAMMPS *lmp, int narg, char **arg)
    : Fix(lmp, narg, arg), ctxp(nullptr), pair_linked(nullptr), pair_mask(nullptr), downloads(0), hostcheck(0), took_delay(0), saved_delay(0),
      linked_to(nullptr), bricks(0), bricks_kw(0), bctx(nullptr), bricks_slot(nullptr), bricks_ev(nullptr), style_id(0), comm_up(0), pending_final(0), step_ev(0)
{
  if (narg < 3 || (narg - 3) % 2) error->all(FLERR, "Illegal fix nve/mdp command");
  if (igroup < 0)
    error->all(FLERR, std::string("Fix ") + arg[2] + " requires group all or a group defined by the group command: could not find fix group ID " + arg[1]);
  if (grouped() && group->count(igroup) == 0)
    error->all(FLERR, std::string("Fix ") + arg[2] + ": group " + arg[1] + " is empty: there is no atom to integrate");
  for (int k = 3; k + 1 < narg; k += 2) {
    const std::string key = arg[k], val = arg[k + 1];
    if ((key != "hostcheck" && key != "bricks") || (val != "yes" && val != "no")) error->all(FLERR, "Illegal fix nve/mdp command");
    if (key == "hostcheck") hostcheck = val == "yes";
    else bricks_kw = val == "yes";
  }
  time_integrate = 1;
  force_reneighbor = 1;
  next_reneighbor = -1;
}

FixNVEMDP::~FixNVEMDP()
{
  // LAMMPS::destroy() deletes Neighbor and Force (and with it the pair style) BEFORE Modify and its fixes, and a new
  // `pair_style` command replaces the pair object under a fix that lives on: what was extracted from the pair style is
  // touched only while force->pair is still the object it came from
  if (took_delay && neighbor) neighbor->delay = saved_delay;
  const bool pair_alive = force && force->pair && force->pair == linked_to;
  if (pair_alive && pair_linked) *pair_linked = 0;
  if (pair_alive && pair_mask) *pair_mask = 0;
  if (pair_alive && bricks_slot) *bricks_slot = nullptr;
  if (bctx) {
    if (comm_up) (void) mdp_dd_comm_destroy(bctx);
    mdp_destroy(bctx);
  } else if (pair_alive && ctx()) {
    (void) mdp_hnve_off(ctx());
    (void) mdp_integrate_group(ctx(), 0); // (the pair style's context may serve another fix next)
    (void) mdp_langevin_group(ctx(), 0);
  }
}

// Neighbor::init() -- which runs behind Modify::init() -- insists that a non-zero delay be a multiple of `every`
int FixNVEMDP::taken_delay() const
{
  const int every = neighbor->every > 0 ? neighbor->every : 1;
  return kDelayTaken - kDelayTaken % every;
}

void FixNVEMDP::fail(mdp_ctx *c) { error->one(FLERR, std::string("Fix nve/mdp: ") + (c ? mdp_last_error(c) : "no device context")); }

int FixNVEMDP::setmask() { return INITIAL_INTEGRATE | FINAL_INTEGRATE; }

void FixNVEMDP::init()
{
  if (!force->pair) error->all(FLERR, "Fix nve/mdp requires a pair style");
  int dim = 0;
  linked_to = force->pair;
  ctxp = static_cast<mdp_ctx **>(force->pair->extract("mdp_ctx", dim));
  pair_linked = static_cast<int *>(force->pair->extract("mdp_nve_linked", dim));
  pair_mask = static_cast<int *>(force->pair->extract("mdp_nve_mask", dim));
  if (grouped() && group_count() == 0.0) error->all(FLERR, std::string("Fix ") + style + ": group " + group->names[igroup] + " is empty: there is no atom to integrate");
  if (!ctxp || !pair_linked || !pair_mask || !ctx())
    error->all(FLERR, "Fix nve/mdp requires a pair style of this plugin (rebomos or aeam)");
  if (comm->nprocs != 1 || bricks_kw) { // several ranks, or `bricks yes` on one: the library's decomposition runs the steps
    init_bricks();
    return;
  }
  if (mdp_hnve_setup(ctx(), update->dt, force->ftm2v, atom->mass, atom->ntypes) != MDP_OK) fail(ctx());
  *pair_linked = 1; // from the next compute on (the setup compute uploads atoms AND velocities)
  *pair_mask = grouped() ? 1 : 0; // ... and atom->mask (a thermostat on a group switches it on in setup())
  next_reneighbor = -1;
  // `check yes`: the device's displacement check decides (see the head of this file); the host's own look at atom->x --
  // a pass over every owned atom per step, of positions that are not current on the host -- leaves the steps
  if (!hostcheck && neighbor->dist_check) {
    if (!took_delay) saved_delay = neighbor->delay;
    took_delay = 1;
    neighbor->delay = taken_delay();
  }
}

// ---- several ranks: the library's decomposition on a context of the fix's own (see the head of this file) ----------

void FixNVEMDP::init_bricks()
{
  int dim = 0;
  bricks_slot = static_cast<mdp_ctx **>(force->pair->extract("mdp_bricks_ctx", dim));
  bricks_ev = static_cast<int *>(force->pair->extract("mdp_bricks_ev", dim));
  if (!bricks_slot || !bricks_ev) error->all(FLERR, "Fix nve/mdp requires a pair style of this plugin (rebomos or aeam)");
  if (hostcheck) error->all(FLERR, "Fix nve/mdp: hostcheck yes needs the host's arrays current: one MPI rank without `bricks yes`");
  if (!domain->xperiodic || !domain->yperiodic || !domain->zperiodic)
    error->all(FLERR, "Fix nve/mdp on several MPI ranks (or with bricks yes) needs a periodic box");
  // the library numbers its bricks as MPI_Cart_create numbers LAMMPS' default grid (`processors * * * map cart`: the last
  // dimension fastest); another mapping (map xyz, numa, a custom file) would hand every rank another rank's brick
  if ((comm->myloc[0] * comm->procgrid[1] + comm->myloc[1]) * comm->procgrid[2] + comm->myloc[2] != comm->me)
    error->all(FLERR, "Fix nve/mdp on several MPI ranks needs the default mapping of ranks to the processor grid (processors ... map cart)");
  // the context is created once; the style's parameters go to it at every init()
  const mdp_own_context_result own = mdp_own_context(force->pair, comm->me, &bctx);
  if (own.why) error->all(FLERR, std::string("Fix nve/mdp") + own.why);
  if (own.failed && !bctx) error->one(FLERR, "Fix nve/mdp: cannot create a device context");
  if (own.failed) fail(bctx);
  style_id = own.style_id;
  bricks_map = own.map;
  bricks = 1;
  // a step with per-atom tallies is let through only when everything that asks for them reads them on the device
  int asking = 0, on_device = 0;
  for (int i = 0; i < modify->ncompute; i++) {
    const Compute *cp = modify->compute[i];
    if (!cp->peatomflag && !cp->pressatomflag) continue;
    asking++;
    const size_t n = strlen(cp->style);
    if (n > 4 && strcmp(cp->style + n - 4, "/mdp") == 0) on_device++;
  }
  atom_ok = asking > 0 && asking == on_device;
  atom_steps = 0;
  *bricks_slot = nullptr; // (the setup compute of this run is the host's: its arrays are the current ones)
  // neither a check nor a reneighboring of the host's during the run: both read arrays that are not current
  if (!took_delay) saved_delay = neighbor->delay;
  took_delay = 1;
  neighbor->delay = taken_delay();
  next_reneighbor = -1;
}

// how the library switches each kind on for a run that opens at step `first` and closes at `last`
static int on(mdp_ctx *c, const MdpHeatSources &b, long long first, long long)
{
  const int rc = mdp_heat_setup(c, b.count, b.cfg, b.bit);
  return rc != MDP_OK ? rc : mdp_heat_run(c, first); // (step `first` itself is not heated, as Verlet::setup does not call end_of_step)
}
// the forces the context holds now are the setup's, the pair style's alone, and the first kick of the run adds the
// indenters' for step `first` in front of itself -- FixIndent::setup's post_force
static int on(mdp_ctx *c, const MdpIndenters &b, long long first, long long)
{
  const int rc = mdp_indent_setup(c, b.count, b.cfg, b.bit);
  return rc != MDP_OK ? rc : mdp_indent_run(c, first);
}
static int on(mdp_ctx *c, const MdpSprings &b, long long first, long long)
{
  const int rc = mdp_spring_setup(c, b.count, b.cfg, b.bit);
  return rc != MDP_OK ? rc : mdp_spring_run(c, first);
}
static int on(mdp_ctx *c, const MdpGforces &b, long long first, long long)
{
  const int rc = mdp_gforce_setup(c, b.count, b.cfg, b.bit);
  return rc != MDP_OK ? rc : mdp_gforce_run(c, first);
}
static int on(mdp_ctx *c, const MdpLangevinBaths &b, long long first, long long last)
{
  // (several: counts the atoms in two baths, the mask is up)
  const int rc = b.count == 1 ? mdp_langevin_setup(c, &b.cfg[0]) : mdp_langevin_baths(c, b.count, b.cfg, b.bit);
  return rc != MDP_OK ? rc : mdp_langevin_run(c, first, last);
}

// Modify::setup, behind the host's own setup (exchange, borders, lists, forces of step 0 in host mode); then what the
// riding fixes handed over, on the context the steps of this run go through
void FixNVEMDP::setup(int vflag)
{
  setup_steps(vflag);
  mdp_ctx *c = bricks ? bctx : ctx();
  if (!c) fail(nullptr);
  apply_groups(c);
  run_ctx = c;
  riders([&](auto &b, const char *, int (*)(mdp_ctx *), const int *against, const char *refusal) {
    if (!b.count) return;
    if (against && *against) error->all(FLERR, refusal);
    if (on(c, b, (long long) update->beginstep, (long long) update->endstep) != MDP_OK) fail(c);
  });
}

// the riding fixes hand their settings over here (copies of their configs; no pointer to any of them is kept)
void *FixNVEMDP::extract(const char *name, int &dim)
{
  dim = 0;
  void *block = nullptr;
  riders([&](auto &b, const char *key, int (*)(mdp_ctx *), const int *, const char *) {
    if (strcmp(name, key) == 0) block = &b;
  });
  if (block) return block;
  if (strcmp(name, "mdp_steps_ctx") == 0) return &run_ctx;
  if (strcmp(name, "mdp_bricks") == 0) return &bricks;
  if (strcmp(name, "mdp_bricks_want") == 0) {
    bricks_want = comm->nprocs != 1 || bricks_kw;
    return &bricks_want;
  }
  return nullptr;
}

bool FixNVEMDP::masked()
{
  bool any = grouped();
  riders([&](auto &b, const char *, int (*)(mdp_ctx *), const int *, const char *) { any = any || b.masked(); });
  return any;
}

double FixNVEMDP::group_count() { return grouped() ? (double) group->count(igroup) : (double) atom->natoms; }

bool FixNVEMDP::brick_mask() { return masked() || mdp_host_has_groups(group); }

// The groups of this run on the context its steps go through.  Group all (and no thermostat on a group): both bits 0, the
// kernels of a context without groups.  Host-linked: the setup compute that has just run uploaded the atoms of this step;
// their mask follows here, and PairMDP::upload_host re-uploads it at every later reneighboring of the host.
void FixNVEMDP::apply_groups(mdp_ctx *c)
{
  if (!bricks) {
    *pair_mask = masked() ? 1 : 0;
    static const int none = 0;
    if (masked() && mdp_hnve_set_mask(c, atom->nlocal ? atom->mask : &none) != MDP_OK) fail(c);
  }
  if (mdp_integrate_group(c, grouped() ? groupbit : 0) != MDP_OK) fail(c);
  if (mdp_langevin_group(c, baths.count == 1 ? baths.bit[0] : 0) != MDP_OK) fail(c); // (several baths bring their bits along)
}

void FixNVEMDP::setup_steps(int vflag)
{
  if (!bricks) return;
  // step 0 with per-atom tallies when LAMMPS opened its setup that way (a compute heatflux/mdp is due): energy and virial
  // with them, as on every such step
  const int at = atom_step(vflag) ? 1 : 0, ef = at ? 3 : 0, vf = at ? 5 : 0;
  atom_steps += at;
  brick_masked = brick_mask() ? 1 : 0;
  if (mdp_brick_from_host(bctx, style_id, bricks_map, atom, domain, force, neighbor, update, comm, brick_masked != 0) != MDP_OK) fail(bctx);
  if (comm->nprocs == 1) { // one brick: its periodic images are the library's, no communicator
    if (mdp_dd_reneighbor(bctx) != MDP_OK) fail(bctx);
    if (mdp_md_compute(bctx, ef, vf) != MDP_OK) fail(bctx);
    pending_final = 0;
    *bricks_slot = bctx;
    return;
  }
  if (!comm_up) { // RCCL's unique id: rank 0 makes it, MPI hands it round
    unsigned char uid[128];
    memset(uid, 0, sizeof uid);
    int ok = 1;
    if (comm->me == 0) ok = mdp_dd_comm_unique_id(uid) == MDP_OK;
    MPI_Bcast(uid, (int) sizeof uid, MPI_BYTE, 0, world);
    if (!ok) error->one(FLERR, "Fix nve/mdp: no RCCL library could be loaded");
    if (mdp_dd_comm_init(bctx, uid) != MDP_OK) fail(bctx);
    comm_up = 1;
  }
  if (mdp_dd_comm_reneighbor(bctx) != MDP_OK) fail(bctx);
  // forces of step 0 for the first half-kick (the host printed its own setup thermo from its host-mode compute)
  int rc;
  if (style_id == 2) {
    rc = mdp_md_aeam_density(bctx, ef);
    if (rc == MDP_OK) rc = mdp_dd_comm_forward_scalar(bctx);
    if (rc == MDP_OK) rc = mdp_md_aeam_force(bctx, ef, vf);
    if (rc == MDP_OK) rc = mdp_dd_comm_reverse(bctx);
  } else
    rc = mdp_md_compute(bctx, ef, vf);
  if (rc != MDP_OK) fail(bctx);
  pending_final = 0;
  *bricks_slot = bctx; // from now on Pair::compute ends the steps this fix opens
}

// the atoms the brick owns NOW, in the brick's order, into the host's arrays
void FixNVEMDP::bricks_to_host()
{
  if (mdp_brick_to_host(bctx, atom, brick_masked != 0) != MDP_OK) fail(bctx);
  downloads++;
}

void FixNVEMDP::reset_dt()
{
  if (bricks) {
    if (bricks_slot && *bricks_slot) error->all(FLERR, "Fix nve/mdp on several MPI ranks: the timestep cannot change during a run");
    return; // (setup() hands update->dt to the brick)
  }
  if (ctx() && mdp_hnve_setup(ctx(), update->dt, force->ftm2v, atom->mass, atom->ntypes) != MDP_OK) fail(ctx());
}

void FixNVEMDP::to_host(bool forces)
{
  const int n = atom->nlocal;
  if (mdp_hnve_download(ctx(), n ? atom->x[0] : nullptr, n ? atom->v[0] : nullptr, (forces && n) ? atom->f[0] : nullptr) != MDP_OK)
    fail(ctx());
  downloads++;
}

void FixNVEMDP::initial_integrate(int vflag)
{
  if (bricks) {
    const bigint now = update->ntimestep;
    step_ev = (vflag || now == output->next || now == update->laststep) ? 1 : 0;
    const int at = atom_step(vflag) ? 1 : 0; // (VIRIAL_ATOM: vflag != 0, so the step has energy and virial too)
    atom_steps += at;
    *bricks_ev = step_ev | (comm->nprocs == 1 ? 2 : 0) | (at ? 4 : 0);
    if (comm->nprocs == 1) { // one brick: the deferred on-device `check yes` flag, the lists rebuilt on the device when it fired
      int moved = 0, dangerous = 0;
      if (mdp_md_integrate_check(bctx, pending_final, &moved, &dangerous) != MDP_OK) fail(bctx);
      if (moved) {
        if (mdp_dd_reneighbor(bctx) != MDP_OK) fail(bctx);
        one_rank_builds++;
      }
    } else {
      int ren = 0;
      if (mdp_dd_comm_step_begin(bctx, pending_final, -1, step_ev | (at ? 2 : 0), step_ev | (at ? 4 : 0), &ren) != MDP_OK) fail(bctx);
    }
    pending_final = step_ev ? 0 : 1; // (Pair::compute ends the step with the half-kick deferred on steps without output)
    return;
  }
  int moved = 0, dangerous = 0;
  if (mdp_hnve_initial(ctx(), &moved, &dangerous) != MDP_OK) fail(ctx());
  const bigint now = update->ntimestep;
  if (getenv("MDP_DEBUG")) fprintf(stderr, "[fix nve/mdp] step %ld moved %d dangerous %d next_reneighbor %ld ago %d\n", (long) now, moved, dangerous, (long) next_reneighbor, neighbor->ago);
  if (moved && next_reneighbor < now) next_reneighbor = now + 1; // (a request for THIS step stands: decide() has not seen it yet)
  // will Neighbor::decide() of this step reneighbor, or read atom->x to find out?  Then the host needs x (and, for the
  // exchange of atoms between the periodic faces, v) now.  (Not under `check yes` without `hostcheck yes`: delay was raised.)
  const int ago = neighbor->ago + 1;
  const bool host_looks = ago >= neighbor->delay && ago % neighbor->every == 0;
  if (next_reneighbor == now || host_looks) to_host(false);
}

// MDP_FIX_STATS=1: one line per run on how often the host's x / v were brought up to date (bench.py reads it)
void FixNVEMDP::post_run()
{
  riders([&](auto &b, const char *, int (*off)(mdp_ctx *), const int *, const char *) { // (an unfix of them gives plain NVE next run)
    if (b.count && run_ctx && off(run_ctx) != MDP_OK) fail(run_ctx);
    b = {};
  });
  run_ctx = nullptr;
  if (bricks) {
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (comm->nprocs > 1) (void) mdp_dd_comm_step_info(bctx, info);
    else info[3] = one_rank_builds;
    one_rank_builds = 0;
    if (comm->me == 0 && getenv("MDP_FIX_STATS"))
      printf("fix nve/mdp: %d bricks, %lld reneighborings on the device, %ld returns of the atoms to the host, %ld computes with per-atom "
             "tallies in this run\n", comm->nprocs, info[3], downloads, atom_steps);
    downloads = 0;
    atom_steps = 0;
    *bricks_slot = nullptr; // the next run's setup is the host's again, from the arrays the last step brought back
    return;
  }
  if (comm->me == 0 && getenv("MDP_FIX_STATS"))
    printf("fix nve/mdp: %ld downloads of x and v in this run (reneighborings the device asked for, output steps, the last step)%s\n",
           downloads, took_delay ? "; check yes decided on the device" : "");
  downloads = 0;
}

void FixNVEMDP::final_integrate()
{
  if (bricks) { // (the half-kick is the library's: in mdp_dd_comm_step_end, or fused into the next step's begin)
    const bigint now = update->ntimestep;
    if (now == output->next || now == update->laststep) bricks_to_host();
    return;
  }
  if (mdp_hnve_final(ctx()) != MDP_OK) fail(ctx());
  const bigint now = update->ntimestep;
  if (now == output->next || now == update->laststep) to_host(false); // thermo, dumps, the state a run ends with
}
