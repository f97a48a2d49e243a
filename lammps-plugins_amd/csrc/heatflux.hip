// heatflux.hip -- the heat current of a device-resident run (LAMMPS compute heat/flux fed ke/atom, pe/atom and
// stress/atom NULL virial):
//   J = sum_i (ke_i + pe_i) v_i + sum_i W_i . v_i
// with pe_i = eatom and W_i = vatom (xx yy zz xy xz yz) as the last compute left them on the device.  Nothing per atom
// crosses the link: one pass over the owned atoms leaves per-block partials in fixed slots and one workgroup adds the
// slots in a fixed order (mdp_block_sum_256 / mdp_slot_sum_256, as msd.hip): no float atomics, two reads of one state
// agree bit for bit.  The sums are extensive (not divided by the volume); the caller adds over ranks.
// The tallies are only what they claim to be right behind a compute that took them (MDP_EFLAG_ATOM and MDP_VFLAG_ATOM):
// the context remembers the flags of its last finished compute and forgets them when a compute starts, the atoms move
// or are re-ordered (mdp_common.h tally_eflag / tally_vflag), and both reads here refuse anything else.
#include "mdp_common.h"

namespace {

// part[kHfW b + k]: block b's sums of (ke + pe) v (3), W.v (3), 1 and ke + pe over the group's atoms.  An atom outside
// the group, and a lane beyond n, adds 0 and still reaches the block sum.  About 100 bytes per atom: v (24), m (8),
// eatom (8), the mask (4) and the 48-byte vatom record as three 16-byte loads.
__global__ __launch_bounds__(256) void heatflux_partial_kernel(const int n, const int gbit, const double hmvv2e,
                                                               const int *__restrict__ mask, const double *__restrict__ rmass,
                                                               const double *__restrict__ v, const double *__restrict__ eatom,
                                                               const double2 *__restrict__ vatom2, double *__restrict__ part)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  double e[kHfW] = {};
  bool in = i < n;
  if (in && gbit) in = (mask[i] & gbit) != 0;
  if (in) {
    const double vx = v[3 * (size_t) i], vy = v[3 * (size_t) i + 1], vz = v[3 * (size_t) i + 2];
    const double2 w01 = vatom2[3 * (size_t) i], w23 = vatom2[3 * (size_t) i + 1], w45 = vatom2[3 * (size_t) i + 2];
    const double en = hmvv2e * rmass[i] * (vx * vx + vy * vy + vz * vz) + eatom[i];
    e[0] = en * vx;
    e[1] = en * vy;
    e[2] = en * vz;
    e[3] = w01.x * vx + w23.y * vy + w45.x * vz; // xx vx + xy vy + xz vz
    e[4] = w23.y * vx + w01.y * vy + w45.y * vz; // xy vx + yy vy + yz vz
    e[5] = w45.x * vx + w45.y * vy + w23.x * vz; // xz vx + yz vy + zz vz
    e[6] = 1.0;
    e[7] = en;
  }
  mdp_block_sum_256<kHfW>(e, part);
}

// both reads: a resident context whose last finished compute took eatom and vatom for the atoms as they are now
int heatflux_require(mdp_ctx *c, const char *who)
{
  if (!c) return MDP_EINVAL;
  if (!c->md) return mdp_fail(c, MDP_ESTATE, "mdp_md_setup not called");
  if (c->tally_eflag < 0 || c->tally_vflag < 0)
    return mdp_fail(c, MDP_ESTATE, "%s: the per-atom tallies are stale: no compute has finished since the atoms last moved, were "
                                   "re-ordered or set up (run the step with MDP_EFLAG_ATOM and MDP_VFLAG_ATOM)", who);
  if (!(c->tally_eflag & MDP_EFLAG_ATOM) || !(c->tally_vflag & MDP_VFLAG_ATOM))
    return mdp_fail(c, MDP_ESTATE, "%s: the last compute ran with eflag %d, vflag %d: per-atom energy and virial need MDP_EFLAG_ATOM "
                                   "and MDP_VFLAG_ATOM", who, c->tally_eflag, c->tally_vflag);
  if (c->cfg.style == 2 && c->dd.on && c->dd.G.nranks > 1 && c->aeam_ang_remote)
    return mdp_fail(c, MDP_ENOTIMPL, "%s: angular centres of this brick reach remote ghosts: the thirds of the per-atom virial they "
                                     "put there would need a reverse exchange between the %d ranks, which is not implemented",
                    who, c->dd.G.nranks);
  MDP_HIP(c, hipSetDevice(c->device));
  return MDP_OK;
}

} // namespace

extern "C" {

int mdp_heatflux_sums(mdp_ctx *c, int groupbit, double out[8])
{
  MDP_TRY(heatflux_require(c, "mdp_heatflux_sums"));
  if (!out) return MDP_EINVAL;
  MDP_TRY(mdp_require_group_mask(c, "mdp_heatflux_sums", groupbit, true));
  MDP_TRY(mdp_md_flush_final(c)); // full-step velocities (a final half is no compute and moves no atom: the tallies stand)
  MdpHeatflux &h = c->heatflux;
  hipStream_t st = c->stream;
  const int n = c->nlocal, nb = n ? nblk(n) : 0;
  MDP_HIP(c, h.part.reserve((size_t) kHfW * (nb + 1)));
  double *tot = h.part.p + (size_t) kHfW * nb;
  if (n)
    heatflux_partial_kernel<<<nb, 256, 0, st>>>(n, groupbit, 0.5 * c->cfg.mvv2e, groupbit ? c->mask.p : nullptr, c->rmass.p, c->v.p,
                                                c->eatom.p, reinterpret_cast<const double2 *>(c->vatom.p), h.part.p);
  mdp_slot_total_kernel<kHfW><<<1, 256, 0, st>>>(h.part.p, nb, tot);
  MDP_HIP(c, hipGetLastError());
  return mdp_read_one(c, tot, sizeof(double) * kHfW, out);
}

int mdp_md_download_vatom(mdp_ctx *c, double *vatom)
{
  MDP_TRY(heatflux_require(c, "mdp_md_download_vatom"));
  if (!vatom) return MDP_EINVAL;
  const int n = c->nlocal;
  if (n) MDP_HIP(c, hipMemcpyAsync(vatom, c->vatom.p, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, c->stream));
  MDP_HIP(c, hipStreamSynchronize(c->stream));
  return MDP_OK;
}

} // extern "C"
