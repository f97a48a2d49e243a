// profile.hip -- binned mass, momentum and kinetic energy of a device-resident run (LAMMPS compute chunk/atom bin/1d|2d|3d
// with temp/chunk, vcm/chunk, fix ave/chunk), in integers.
// An owned atom falls into the row its fractional coordinates name (dd_x2lamda in the box of mdp_dd_setup: triclinic boxes
// included); its terms t = (m, m vx, m vy, m vz, m v.v) are scaled by a power of two per column that the CALLER derives from
// the global maximum of |t_k| (mdp_profile_range, mdp_profile_exponent), rounded to 64-bit integers and added with integer
// atomics: while the table fits, into a per-workgroup copy in LDS whose non-zero entries go to the global table once; above
// that, straight into the global table (the atoms are cell-ordered, so a wave's adds fall on few rows).  Integer sums do not
// depend on their order: two reads of one state agree exactly, and the sum over the bricks of a decomposition is the
// one-brick table bit for bit.  No floating-point atomic anywhere.  One grid-stride pass each; nothing a step, a list build,
// msd or rdf reads is written.
#include "mdp_common.h"

#include <cmath>

namespace {

constexpr int kProfW = MDP_PROFILE_W;
constexpr int kProfLdsWords = 4096; // rows * kProfW 64-bit sums a workgroup keeps in LDS (32 KB), with rows 32-bit counts
constexpr int kProfMaxGrid = 2048;  // workgroups of a pass

struct ProfBins {
  int ndim, dim[3], nbin[3];
};

// the terms of one atom: written once, so the range and the sums see the same bits (mdp_dot3 fixes the roundings of v . v)
__device__ __forceinline__ void profile_terms(const double m, const double *__restrict__ v, double t[kProfW])
{
  const double vx = v[0], vy = v[1], vz = v[2];
  t[0] = m;
  t[1] = m * vx;
  t[2] = m * vy;
  t[3] = m * vz;
  t[4] = m * mdp_dot3(vx, vx, vy, vy, vz, vz);
}

// row of a position: b_d = floor(s_d n_d), wrapped in a periodic dimension, clamped in a non-periodic one; the first named
// dimension slowest.  Always inside 0 .. rows - 1, whatever the position holds (fmax / fmin drop a NaN).
__device__ __forceinline__ int profile_row(const DdGeom &G, const ProfBins &P, const double4 &x)
{
  double lam[3];
  dd_x2lamda(G, x.x, x.y, x.z, lam);
  int row = 0;
  for (int k = 0; k < P.ndim; k++) {
    const int d = P.dim[k], n = P.nbin[k];
    const double f = floor(lam[d] * (double) n);
    int b = (int) fmin(fmax(f, -1.0e9), 1.0e9);
    if (G.nonper[d])
      b = b < 0 ? 0 : (b >= n ? n - 1 : b);
    else
      b = ((b % n) + n) % n;
    row = row * n + b;
  }
  return row;
}

__device__ __forceinline__ bool profile_member(const int i, const int gbit, const int *__restrict__ mask)
{ return !gbit || (mask[i] & gbit) != 0; }

// part[kProfW b + k] = the maximum of e[k] over the lanes of workgroup b (every lane must call it; e >= 0)
__device__ __forceinline__ void profile_block_max(const double e[kProfW], double *__restrict__ part)
{
  __shared__ double wmax[kProfW][4];
#pragma unroll
  for (int k = 0; k < kProfW; k++) {
    double s = e[k];
    for (int o = 32; o > 0; o >>= 1) s = fmax(s, __shfl_xor(s, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < kProfW) part[kProfW * (size_t) blockIdx.x + k] = fmax(fmax(wmax[k][0], wmax[k][1]), fmax(wmax[k][2], wmax[k][3]));
}

__global__ __launch_bounds__(256) void profile_range_kernel(const int n, const int gbit, const int *__restrict__ mask,
                                                            const double *__restrict__ rmass, const double *__restrict__ v,
                                                            double *__restrict__ part)
{
  double e[kProfW] = {};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if (!profile_member(i, gbit, mask)) continue;
    double t[kProfW];
    profile_terms(rmass[i], v + 3 * (size_t) i, t);
#pragma unroll
    for (int k = 0; k < kProfW; k++) e[k] = fmax(e[k], fabs(t[k]));
  }
  profile_block_max(e, part);
}

// ONE workgroup: out[k] = the maximum over the npart slots
__global__ __launch_bounds__(256) void profile_range_total_kernel(const double *__restrict__ part, const int npart,
                                                                  double *__restrict__ out)
{
  double e[kProfW] = {};
  for (int b = threadIdx.x; b < npart; b += 256)
#pragma unroll
    for (int k = 0; k < kProfW; k++) e[k] = fmax(e[k], part[kProfW * (size_t) b + k]);
  profile_block_max(e, out);
}

// Dynamic LDS with LDS: [0, rows * kProfW) the 64-bit sums, then rows 32-bit counts.  out: [rows][kProfW] sums, [rows] counts,
// then one word of column flags (bit k: a scaled term of column k reached lim = 2^62 / max(nlocal, 1)).
template <bool LDS>
__global__ __launch_bounds__(256) void profile_sums_kernel(const DdGeom G, const ProfBins P, const int rows, const int n,
                                                           const int gbit, const int e0, const int e1, const int e2,
                                                           const int e3, const int e4, const double lim,
                                                           const double4 *__restrict__ xq, const int *__restrict__ mask,
                                                           const double *__restrict__ rmass, const double *__restrict__ v,
                                                           unsigned long long *__restrict__ out)
{
  extern __shared__ __attribute__((aligned(16))) unsigned long long prof_lds[];
  const int nsum = rows * kProfW;
  unsigned long long *ls = prof_lds;
  unsigned *lc = (unsigned *) (prof_lds + nsum);
  if (LDS) {
    for (int k = threadIdx.x; k < nsum; k += 256) ls[k] = 0ull;
    for (int k = threadIdx.x; k < rows; k += 256) lc[k] = 0u;
    __syncthreads();
  }
  const int ex[kProfW] = {e0, e1, e2, e3, e4};
  unsigned bad = 0u;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if (!profile_member(i, gbit, mask)) continue;
    double t[kProfW];
    profile_terms(rmass[i], v + 3 * (size_t) i, t);
    long long q[kProfW];
    unsigned mybad = 0u;
#pragma unroll
    for (int k = 0; k < kProfW; k++) {
      const double s = ldexp(t[k], ex[k]);
      if (!(fabs(s) < lim)) { // (a NaN too)
        mybad |= 1u << k;
        q[k] = 0;
      } else
        q[k] = llrint(s);
    }
    if (mybad) { // the read is refused: the atom is left out
      bad |= mybad;
      continue;
    }
    const int row = profile_row(G, P, xq[i]);
    if (LDS) {
      atomicAdd(lc + row, 1u);
#pragma unroll
      for (int k = 0; k < kProfW; k++)
        if (q[k]) atomicAdd(ls + row * kProfW + k, (unsigned long long) q[k]);
    } else {
      atomicAdd(out + (size_t) nsum + row, 1ull);
#pragma unroll
      for (int k = 0; k < kProfW; k++)
        if (q[k]) atomicAdd(out + (size_t) row * kProfW + k, (unsigned long long) q[k]);
    }
  }
  if (bad) atomicOr(out + (size_t) nsum + rows, (unsigned long long) bad);
  if (LDS) {
    __syncthreads();
    for (int k = threadIdx.x; k < nsum; k += 256)
      if (ls[k]) atomicAdd(out + k, ls[k]);
    for (int k = threadIdx.x; k < rows; k += 256)
      if (lc[k]) atomicAdd(out + (size_t) nsum + k, (unsigned long long) lc[k]);
  }
}

int profile_require(mdp_ctx *c, const char *who)
{
  if (!c) return MDP_EINVAL;
  if (!c->md) return mdp_fail(c, MDP_ESTATE, "mdp_md_setup not called");
  if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "%s: mdp_dd_setup not called (the bins are fractions of the box of the brick)", who);
  MDP_HIP(c, hipSetDevice(c->device));
  return MDP_OK;
}

// a read: the setup is there, the mask covers the atoms, and the velocities are those of the full step
int profile_open(mdp_ctx *c, const char *who)
{
  MDP_TRY(profile_require(c, who));
  const MdpProfile &h = c->profile;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_profile_setup not called");
  MDP_TRY(mdp_require_group_mask(c, who, h.gbit, true));
  return mdp_md_flush_final(c);
}

// the workgroups of a pass: the range is a maximum and the sums are integers, so any grid reads the same bits (the test
// hook MDP_MEASURE_GRID lowers it)
int profile_grid(const int n) { return mdp_measure_grid(nblk(n), kProfMaxGrid); }

} // namespace

static void profile_release(mdp_ctx *c) // mdp_profile_off: the measurement's buffers go ahead of the context's end
{
  c->profile.part.release();
  c->profile.out.release();
  c->profile.on = false;
}

extern "C" {

int mdp_profile_setup(mdp_ctx *c, int ndim, const int *dim, const int *nbin, int groupbit)
{
  MDP_TRY(profile_require(c, "mdp_profile_setup"));
  if (ndim < 1 || ndim > 3) return mdp_fail(c, MDP_EINVAL, "mdp_profile_setup: ndim must be 1 .. 3, not %d", ndim);
  if (!dim || !nbin) return mdp_fail(c, MDP_EINVAL, "mdp_profile_setup: no dimensions");
  long long rows = 1;
  for (int k = 0; k < ndim; k++) {
    if (dim[k] < 0 || dim[k] > 2) return mdp_fail(c, MDP_EINVAL, "mdp_profile_setup: dimension %d is not 0, 1 or 2", dim[k]);
    for (int j = 0; j < k; j++)
      if (dim[j] == dim[k]) return mdp_fail(c, MDP_EINVAL, "mdp_profile_setup: dimension %d is named twice", dim[k]);
    if (nbin[k] < 1) return mdp_fail(c, MDP_EINVAL, "mdp_profile_setup: nbin must be >= 1, not %d", nbin[k]);
    rows *= nbin[k]; // (each factor below 2^31 and the product checked after every one: no overflow)
    if (rows > MDP_PROFILE_MAXBINS)
      return mdp_fail(c, MDP_EINVAL, "mdp_profile_setup: more than %d rows", MDP_PROFILE_MAXBINS);
  }
  MDP_TRY(mdp_require_group_mask(c, "mdp_profile_setup", groupbit, false));
  MdpProfile &h = c->profile;
  MDP_HIP(c, h.out.reserve((size_t) rows * (kProfW + 1) + 1));
  h.ndim = ndim;
  for (int k = 0; k < 3; k++) {
    h.dim[k] = k < ndim ? dim[k] : 0;
    h.nbin[k] = k < ndim ? nbin[k] : 1;
  }
  h.rows = rows;
  h.gbit = groupbit;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_profile_range(mdp_ctx *c, double out[MDP_PROFILE_W])
{
  if (c && !out) return MDP_EINVAL;
  MDP_TRY(profile_open(c, "mdp_profile_range"));
  MdpProfile &h = c->profile;
  hipStream_t st = c->stream;
  const int n = c->nlocal, nb = n ? profile_grid(n) : 0;
  MDP_HIP(c, h.part.reserve((size_t) kProfW * (nb + 1)));
  double *tot = h.part.p + (size_t) kProfW * nb;
  if (n) profile_range_kernel<<<nb, 256, 0, st>>>(n, h.gbit, h.gbit ? c->mask.p : nullptr, c->rmass.p, c->v.p, h.part.p);
  profile_range_total_kernel<<<1, 256, 0, st>>>(h.part.p, nb, tot);
  MDP_HIP(c, hipGetLastError());
  return mdp_read_one(c, tot, sizeof(double) * kProfW, out);
}

int mdp_profile_exponent(double range, long long natoms_total)
{
  if (!(range > 0.0) || !std::isfinite(range)) return 0;
  int E = 0;
  (void) frexp(range, &E); // range = f 2^E, 0.5 <= f < 1
  const long long n = natoms_total > 2 ? natoms_total : 2;
  int L = 1;
  while (L < 62 && (1ll << L) < n) L++;
  return 61 - L - E;
}

int mdp_profile_sums(mdp_ctx *c, const int exponent[MDP_PROFILE_W], long long *count, long long *sums)
{
  if (c && (!exponent || !count || !sums)) return MDP_EINVAL;
  MDP_TRY(profile_open(c, "mdp_profile_sums"));
  MdpProfile &h = c->profile;
  hipStream_t st = c->stream;
  const int n = c->nlocal, rows = (int) h.rows;
  const size_t nsum = (size_t) rows * kProfW, nout = nsum + rows + 1;
  MDP_HIP(c, h.out.reserve(nout));
  MDP_HIP(c, hipMemsetAsync(h.out.p, 0, sizeof(unsigned long long) * nout, st));
  if (n) {
    ProfBins P;
    P.ndim = h.ndim;
    for (int k = 0; k < 3; k++) {
      P.dim[k] = h.dim[k];
      P.nbin[k] = h.nbin[k];
    }
    const double lim = ldexp(1.0, 62) / (double) n;
    const int *mask = h.gbit ? c->mask.p : nullptr, *e = exponent;
    const int grid = profile_grid(n);
    if (nsum <= (size_t) kProfLdsWords) {
      const size_t lds = sizeof(unsigned long long) * nsum + sizeof(unsigned) * rows;
      profile_sums_kernel<true><<<grid, 256, lds, st>>>(c->dd.G, P, rows, n, h.gbit, e[0], e[1], e[2], e[3], e[4], lim, c->xq.p, mask,
                                                        c->rmass.p, c->v.p, h.out.p);
    } else
      profile_sums_kernel<false><<<grid, 256, 0, st>>>(c->dd.G, P, rows, n, h.gbit, e[0], e[1], e[2], e[3], e[4], lim, c->xq.p, mask,
                                                       c->rmass.p, c->v.p, h.out.p);
    MDP_HIP(c, hipGetLastError());
  }
  unsigned long long flags = 0;
  const MdpRead r[3] = {{h.out.p, sizeof(long long) * nsum, sums},
                        {h.out.p + nsum, sizeof(long long) * rows, count},
                        {h.out.p + nsum + rows, sizeof flags, &flags}};
  MDP_TRY(mdp_read_small(c, r, 3));
  if (flags) {
    static const char *const name[kProfW] = {"m", "m vx", "m vy", "m vz", "m v^2"};
    int k = 0;
    while (!(flags >> k & 1ull)) k++;
    return mdp_fail(c, MDP_EINVAL, "mdp_profile_sums: column %d (%s): a term scaled by 2^%d reaches 2^62 / %d atoms, the 64-bit sum could "
                                   "overflow: take the exponent from mdp_profile_exponent of the global mdp_profile_range",
                    k, name[k], exponent[k], n > 1 ? n : 1);
  }
  return MDP_OK;
}

int mdp_profile_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->profile, c->profile.rows, c->profile.ndim, out);
}

int mdp_profile_off(mdp_ctx *c) { return mdp_measure_off(c, profile_release); }

} // extern "C"
