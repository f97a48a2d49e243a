// msd.hip -- unwrapped positions and the mean-squared displacement of a device-resident run (LAMMPS compute msd).
// The image flag of an owned atom (mdp_md_set_image) counts the box vectors the remap of domain.hip has taken off it, so
//   xu = x + h . image
// is where the atom would be had it never been wrapped.  The origins xu(0) are kept for the WHOLE system on every rank,
// indexed by tag: an atom that migrates finds its origin on its new rank, and nothing has to travel.
// The sums of a read are one pass over the owned atoms that leaves per-block partials in fixed slots and one workgroup
// that adds the slots in a fixed order (mdp_block_sum_256 / mdp_slot_sum_256): no float atomics, two reads of one state
// agree bit for bit.  The caller divides, and on several ranks sums over the ranks first.
#include "mdp_common.h"

namespace {

__global__ __launch_bounds__(256) void msd_unwrap_kernel(const DdGeom G, const int n, const double4 *__restrict__ xq,
                                                         const int *__restrict__ image, double *__restrict__ xu)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double u[3];
  mdp_unwrap(G, xq[i], image[i], u);
  xu[3 * (size_t) i] = u[0];
  xu[3 * (size_t) i + 1] = u[1];
  xu[3 * (size_t) i + 2] = u[2];
}

// origins from the current state: x0[tag - 1] = xu of the owned atom with that tag (one rank: every tag is owned)
__global__ __launch_bounds__(256) void msd_origin_kernel(const DdGeom G, const int n, const int ntag,
                                                         const double4 *__restrict__ xq, const int *__restrict__ image,
                                                         const int *__restrict__ tag, double *__restrict__ x0)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int t = tag[i];
  if (t < 1 || t > ntag) return; // (mdp_msd_sums reports such an atom)
  double u[3];
  mdp_unwrap(G, xq[i], image[i], u);
  x0[3 * (size_t) (t - 1)] = u[0];
  x0[3 * (size_t) (t - 1) + 1] = u[1];
  x0[3 * (size_t) (t - 1) + 2] = u[2];
}

// part[kMsdW b + k]: block b's sums of dx^2, dy^2, dz^2, 1, m xu (3), m over the group's atoms, d = (xu - x0[tag - 1]) - shift,
// and the count of atoms whose tag has no origin.  An atom outside the group, and a lane beyond n, adds 0 and still reaches
// the block sum.
__global__ __launch_bounds__(256) void msd_partial_kernel(const DdGeom G, const int n, const int ntag, const int gbit,
                                                          const double4 *__restrict__ xq, const int *__restrict__ image,
                                                          const int *__restrict__ tag, const int *__restrict__ mask,
                                                          const double *__restrict__ rmass, const double *__restrict__ x0,
                                                          const double sx, const double sy, const double sz,
                                                          double *__restrict__ part)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  double e[kMsdW] = {};
  bool in = i < n;
  if (in && gbit) in = (mask[i] & gbit) != 0;
  if (in) {
    const int t = tag[i];
    if (t < 1 || t > ntag) {
      e[8] = 1.0;
    } else {
      double u[3];
      mdp_unwrap(G, xq[i], image[i], u);
      const double *o = x0 + 3 * (size_t) (t - 1);
      const double dx = (u[0] - o[0]) - sx, dy = (u[1] - o[1]) - sy, dz = (u[2] - o[2]) - sz, m = rmass[i];
      e[0] = dx * dx;
      e[1] = dy * dy;
      e[2] = dz * dz;
      e[3] = 1.0;
      e[4] = m * u[0];
      e[5] = m * u[1];
      e[6] = m * u[2];
      e[7] = m;
    }
  }
  mdp_block_sum_256<kMsdW>(e, part);
}

int msd_require(mdp_ctx *c, const char *who)
{
  if (!c) return MDP_EINVAL;
  if (!c->md) return mdp_fail(c, MDP_ESTATE, "mdp_md_setup not called");
  if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "%s: mdp_dd_setup not called (the unwrapped positions need the box of the brick)", who);
  if (!c->image_set) return mdp_fail(c, MDP_ESTATE, "%s: no image set (mdp_md_set_image)", who);
  MDP_HIP(c, hipSetDevice(c->device));
  return MDP_OK;
}

} // namespace

static void msd_release(mdp_ctx *c) // mdp_msd_off: the measurement's buffers go ahead of the context's end
{
  c->msd.x0.release();
  c->msd.xu.release();
  c->msd.part.release();
  c->msd.on = false;
}

extern "C" {

int mdp_md_download_unwrapped(mdp_ctx *c, double *xu)
{
  MDP_TRY(msd_require(c, "mdp_md_download_unwrapped"));
  if (!xu) return MDP_EINVAL;
  const int n = c->nlocal;
  if (!n) return MDP_OK;
  hipStream_t st = c->stream;
  MDP_HIP(c, c->msd.xu.reserve((size_t) 3 * n + 3));
  msd_unwrap_kernel<<<nblk(n), 256, 0, st>>>(c->dd.G, n, c->xq.p, c->image.p, c->msd.xu.p);
  MDP_HIP(c, hipGetLastError());
  MDP_HIP(c, hipMemcpyAsync(xu, c->msd.xu.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
  MDP_HIP(c, hipStreamSynchronize(st));
  return MDP_OK;
}

int mdp_msd_setup(mdp_ctx *c, int ntag, const double *x0_by_tag, int groupbit)
{
  MDP_TRY(msd_require(c, "mdp_msd_setup"));
  if (ntag < 1) return mdp_fail(c, MDP_EINVAL, "mdp_msd_setup: ntag must be >= 1");
  if (!x0_by_tag && c->dd.G.nranks > 1)
    return mdp_fail(c, MDP_ESTATE, "mdp_msd_setup: origins from the current positions (NULL) are for one rank only; on a brick of %d "
                                   "ranks an arriving atom's origin would be unknown: pass the origins of all atoms by tag",
                    c->dd.G.nranks);
  if (!x0_by_tag && c->nlocal != ntag)
    return mdp_fail(c, MDP_EINVAL, "mdp_msd_setup: origins from the current positions need ntag = the %d owned atoms", c->nlocal);
  MDP_TRY(mdp_require_group_mask(c, "mdp_msd_setup", groupbit, false));
  MdpMsd &h = c->msd;
  hipStream_t st = c->stream;
  MDP_HIP(c, h.x0.reserve((size_t) 3 * ntag + 3));
  if (x0_by_tag) {
    MDP_TRY(mdp_host_upload(c, h.x0.p, x0_by_tag, sizeof(double) * 3 * (size_t) ntag));
  } else {
    MDP_HIP(c, hipMemsetAsync(h.x0.p, 0, sizeof(double) * 3 * (size_t) ntag, st));
    msd_origin_kernel<<<nblk(c->nlocal), 256, 0, st>>>(c->dd.G, c->nlocal, ntag, c->xq.p, c->image.p, c->tag.p, h.x0.p);
    MDP_HIP(c, hipGetLastError());
  }
  MDP_HIP(c, hipStreamSynchronize(st)); // the caller's array may change after return
  h.ntag = ntag;
  h.gbit = groupbit;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_msd_sums(mdp_ctx *c, const double *shift, double out[8])
{
  MDP_TRY(msd_require(c, "mdp_msd_sums"));
  if (!out) return MDP_EINVAL;
  MdpMsd &h = c->msd;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_msd_setup not called");
  MDP_TRY(mdp_require_group_mask(c, "mdp_msd_sums", h.gbit, true));
  hipStream_t st = c->stream;
  const int n = c->nlocal, nb = n ? nblk(n) : 0;
  MDP_HIP(c, h.part.reserve((size_t) kMsdW * (nb + 1)));
  double *tot = h.part.p + (size_t) kMsdW * nb;
  if (n)
    msd_partial_kernel<<<nb, 256, 0, st>>>(c->dd.G, n, h.ntag, h.gbit, c->xq.p, c->image.p, c->tag.p,
                                           h.gbit ? c->mask.p : nullptr, c->rmass.p, h.x0.p, shift ? shift[0] : 0.0,
                                           shift ? shift[1] : 0.0, shift ? shift[2] : 0.0, h.part.p);
  mdp_slot_total_kernel<kMsdW><<<1, 256, 0, st>>>(h.part.p, nb, tot);
  MDP_HIP(c, hipGetLastError());
  double s[kMsdW];
  MDP_TRY(mdp_read_one(c, tot, sizeof s, s));
  if (s[8] != 0.0)
    return mdp_fail(c, MDP_EINVAL, "mdp_msd_sums: %d owned atoms have a tag outside 1 .. %d, the origins of mdp_msd_setup", (int) s[8],
                    h.ntag);
  for (int k = 0; k < 8; k++) out[k] = s[k];
  return MDP_OK;
}

int mdp_msd_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->msd, c->msd.ntag, c->msd.gbit, out);
}

int mdp_msd_off(mdp_ctx *c) { return mdp_measure_off(c, msd_release); }

} // extern "C"
