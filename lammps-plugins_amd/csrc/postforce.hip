// The life cycle that the post-force stages share (kMdpStages, mdp_common.h: the indenters, the tether springs, the group forces):
// what a _setup refuses and commits, _run, the common part of _state, _off, and the refusals of the modules that do not
// go with a stage.  The per-step part (mdp_postforce_apply, mdp_postforce_count_step) is inline in mdp_common.h.  The
// kernels, the passes and the argument checks of a kind stay in its own file (indent.hip, spring.hip, gforce.hip).
#include "mdp_common.h"

#include <cstring>

namespace {

// a stage's _setup / _run: the forces the context holds are taken to be the pair style's alone, those of step `first`
void postforce_restart(MdpPostForce &h, long long first)
{
  h.first = first;
  h.nhalf = 0;
  h.applied = false;
}

} // namespace

int mdp_postforce_refuse_setup(mdp_ctx *c, int s)
{
  const MdpStage &S = kMdpStages[s];
  if (c->fire.on) return mdp_fail(c, MDP_ESTATE, "%s_setup: a minimisation (mdp_fire_setup) is on; mdp_fire_off first", S.api);
  if (c->nhc.on)
    return mdp_fail(c, MDP_ESTATE, "%s_setup: the Nose-Hoover chain (mdp_nhc_setup) is on; %s run under NVE and Langevin baths", S.api, S.many);
  if (c->heat.on) return mdp_fail(c, MDP_ESTATE, "%s_setup: heat sources (mdp_heat_setup) are on; mdp_heat_off first", S.api);
  if (c->dd.on && c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "%s_setup: %s run on one rank only (this context is a brick of %d ranks)", S.api, S.many, c->dd.G.nranks);
  return MDP_OK;
}

int mdp_postforce_commit(mdp_ctx *c, int s, int words, int n, const int *groupbit, void *cfg_dst, const void *cfg, size_t cfg_bytes)
{
  MdpPostForce &h = kMdpStages[s].base(c);
  { // a final half the host deferred belongs to the run before: it completes now, without this stage
    const bool was_on = h.on;
    h.on = false;
    const int rc = mdp_md_flush_final(c);
    if (rc != MDP_OK) {
      h.on = was_on;
      return rc;
    }
  }
  MDP_HIP(c, h.st.reserve(words));
  const double zero[kSprTotal] = {};
  static_assert(kSprTotal >= MDP_INDENT_MAX * MDP_INDENT_STATE_LEN && kSprTotal >= MDP_GFORCE_MAX * MDP_GFORCE_STATE_LEN,
                "the state words of the largest stage");
  MDP_TRY(mdp_write_small(c, h.st.p, zero, sizeof(double) * words));
  h.n = n;
  for (int k = 0; k < kStageSlots; k++) h.bit[k] = k < n ? groupbit[k] : 0;
  memcpy(cfg_dst, cfg, cfg_bytes * n);
  postforce_restart(h, 0);
  h.on = true;
  return MDP_OK;
}

int mdp_postforce_run(mdp_ctx *c, int s, long long first)
{
  MdpPostForce &h = kMdpStages[s].base(c);
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "%s_setup not called", kMdpStages[s].api);
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(mdp_md_flush_final(c)); // (the last kick of the run before, with the passes of its step if they are due)
  postforce_restart(h, first);
  return MDP_OK;
}

int mdp_postforce_state(mdp_ctx *c, int s, int k, int len, double *out)
{
  const MdpStage &S = kMdpStages[s];
  MdpPostForce &h = S.base(c);
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "%s_setup not called", S.api);
  if (k < 0 || k >= h.n) return mdp_fail(c, MDP_EINVAL, "%s_state: %s index %d out of range (%d %s are on)", S.api, S.one, k, h.n, S.many);
  MDP_HIP(c, hipSetDevice(c->device));
  MDP_TRY(mdp_md_flush_final(c));
  // the forces of a step no kick has consumed yet (step `first` before a run): the passes in front of this stage's go
  // first, as in front of a kick; a stage behind it is left for the kick
  if (!h.applied) MDP_TRY(mdp_postforce_apply(c, s));
  return mdp_read_one(c, h.st.p + k * len, sizeof(double) * len, out);
}

int mdp_postforce_off(mdp_ctx *c, int s)
{
  MdpPostForce &h = kMdpStages[s].base(c);
  // a deferred final half of the last step completes with its pass before the plain kicks take over
  if (h.on) MDP_TRY(mdp_md_flush_final(c));
  h.on = false;
  mdp_postforce_release(c, s);
  return MDP_OK;
}

void mdp_postforce_release(mdp_ctx *c, int s)
{
  MdpPostForce &h = kMdpStages[s].base(c);
  h.st.release();
  h.part.release();
  if (s == kStageSpring) {
    c->spring.cpart.release();
    c->spring.count.release();
  }
  if (s == kStageGforce) {
    c->gforce.cpart.release();
    c->gforce.count.release();
  }
}

int mdp_refuse_if_on(mdp_ctx *c, const char *who, MdpRefuse how)
{
  for (const MdpStage &S : kMdpStages) {
    if (!S.base(c).on) continue;
    if (how == kRefuseOffFirst) return mdp_fail(c, MDP_ESTATE, "%s: %s (%s_setup) are on; %s_off first", who, S.many, S.api, S.api);
    return mdp_fail(c, MDP_ESTATE, "%s: %s (%s_setup) run on one rank only, not on a brick of several ranks", who, S.many, S.api);
  }
  return MDP_OK;
}
