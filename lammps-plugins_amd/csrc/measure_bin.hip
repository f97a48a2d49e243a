// measure_bin.hip -- the binning stage of the neighbour measurements (rdf.hip, adf.hip, coord.hip, centro.hip) and what their
// setups and reads share on the host (mdp_measure_*, mdp_hist_*): ALL atoms of the brick, owned and
// ghost, on a grid of the measurement's own at cell width >= cutoff / 2, into the buffers of an MdpBinning.  The list
// builders' grid, permutation, cell starts and cell-ordered positions (mdp_bin_atoms) are neither read nor written, so a
// read changes nothing a later step or list build sees.  What comes out: cell_start and the cell-ordered records
// {x, y, z, code}; the code word carries the type (0 for an atom outside the group) and the owned bit, so one 32-byte load
// per candidate is all the inner loop of a histogram kernel reads.
#include "mdp_common.h"

#include <rocprim/rocprim.hpp>

namespace {

using Grid = MdpGrid;

// key = cell, value = atom; code[i] = (member ? type : 0) | (owned ? kBinOwned : 0).  An atom whose tag has no entry in the
// member table is counted in *bad (the read refuses) and treated as outside the group.
__global__ __launch_bounds__(256) void bin_assign_kernel(const Grid g, const int nall, const int nlocal, const int ntypes,
                                                         const double4 *__restrict__ xq, const int *__restrict__ type,
                                                         const int *__restrict__ tag, const int ntag,
                                                         const unsigned char *__restrict__ member,
                                                         unsigned *__restrict__ key, int *__restrict__ val,
                                                         int *__restrict__ code, unsigned long long *__restrict__ bad)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nall) return;
  int cx, cy, cz;
  key[i] = (unsigned) mdp_bin_cell_index(g, xq[i], cx, cy, cz);
  val[i] = i;
  int t = type[i];
  if (t < 1 || t > ntypes) t = 0; // (a type no column can name)
  if (member) {
    const int tg = tag[i];
    if (tg < 1 || tg > ntag) {
      atomicAdd(bad, 1ull);
      t = 0;
    } else if (!member[tg - 1])
      t = 0;
  }
  code[i] = t | (i < nlocal ? kBinOwned : 0);
}

// cell_start[c] .. cell_start[c + 1] delimit cell c in the sorted order, filled for every cell up to the last occupied
// one (bin_tail_kernel: the rest); rec[p] = {x, y, z, code} of the atom at place p, the code in the low word of w
__global__ __launch_bounds__(256) void bin_bounds_kernel(const int nall, const unsigned *__restrict__ key_sorted,
                                                         const int *__restrict__ perm, const double4 *__restrict__ xq,
                                                         const int *__restrict__ code, int *__restrict__ cell_start,
                                                         double4 *__restrict__ rec)
{
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nall) return;
  const int a = perm[p];
  double4 r = xq[a];
  r.w = __hiloint2double(0, code[a]);
  rec[p] = r;
  const unsigned k = key_sorted[p];
  const unsigned kprev = p == 0 ? 0u : key_sorted[p - 1];
  if (p == 0)
    for (unsigned c = 0; c <= k; c++) cell_start[c] = 0;
  else
    for (unsigned c = kprev + 1; c <= k; c++) cell_start[c] = p;
}

__global__ void bin_tail_kernel(const int nall, const int ncell, const unsigned *__restrict__ key_sorted,
                                int *__restrict__ cell_start)
{
  const unsigned last = key_sorted[nall - 1];
  for (int c = (int) last + 1 + threadIdx.x; c <= ncell; c += blockDim.x) cell_start[c] = nall;
}

// the grid of a read: cells >= cutoff / 2 wide over the padded hull of the brick (mdp_dd_borders_end), and no more cells
// than a few per atom -- wider cells are still correct with the 5-cell stencil
void bin_grid(const mdp_ctx *c, const double cutoff, Grid &g, long long &ncell)
{
  double binsize = 0.5 * cutoff;
  const long long cap = 4ll * c->nall + 4096;
  for (;;) {
    ncell = 1;
    for (int d = 0; d < 3; d++) {
      const double len = c->cfg.bbox_hi[d] - c->cfg.bbox_lo[d];
      int n = (int) floor(len / binsize);
      if (n < 1) n = 1;
      if (n > 1024) n = 1024;
      g.n[d] = n;
      g.lo[d] = c->cfg.bbox_lo[d];
      g.inv[d] = n / len;
      ncell *= n;
    }
    if (ncell <= cap) break;
    binsize *= 1.26;
  }
  g.range = 2;
}

} // namespace

int mdp_measure_require(mdp_ctx *c, const char *who)
{
  if (!c) return MDP_EINVAL;
  if (!c->md) return mdp_fail(c, MDP_ESTATE, "mdp_md_setup not called");
  if (!c->dd.on) return mdp_fail(c, MDP_ESTATE, "%s: mdp_dd_setup not called (the ghost shell of the brick holds the partners)", who);
  MDP_HIP(c, hipSetDevice(c->device));
  return MDP_OK;
}

int mdp_measure_grid(const int nchunk, const int resident)
{
  int grid = nchunk < resident ? nchunk : resident;
  const char *e = getenv("MDP_MEASURE_GRID");
  const int knob = e ? atoi(e) : 0;
  if (knob > 0 && knob < grid) grid = knob;
  return grid;
}

int mdp_measure_resident(mdp_ctx *c, const size_t lds_bytes, int &resident)
{
  if (c->num_cu <= 0) {
    int n = 0;
    MDP_HIP(c, hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device));
    c->num_cu = n > 0 ? n : 256;
  }
  const int fit = (int) ((size_t) 144 * 1024 / lds_bytes);
  resident = (fit < 1 ? 1 : (fit > 8 ? 8 : fit)) * c->num_cu;
  return MDP_OK;
}

int mdp_measure_ntypes(mdp_ctx *c, const char *who, int &ntypes)
{
  // mdp_md_setup admits 1 .. 15 atom types, which is what the 4-bit type code of a record and the 16-entry mask tables hold:
  // the check below cannot fire on a context that passed mdp_measure_require, and stands for a later change of that limit
  ntypes = c->ntypes > 0 ? c->ntypes : c->cfg.ntypes;
  if (ntypes < 1 || ntypes >= kBinTypes)
    return mdp_fail(c, MDP_EINVAL, "%s: %d atom types (the type code of a record holds 1 .. %d)", who, ntypes, kBinTypes - 1);
  return MDP_OK;
}

int mdp_measure_type_ranges(mdp_ctx *c, const char *who, const char *noun, const int index, const int ntypes, const int n, const int *lohi)
{
  for (int k = 0; k < n; k++)
    if (lohi[k] < 1 || lohi[k] > ntypes)
      return mdp_fail(c, MDP_EINVAL, "%s: %s %d: type %d outside 1 .. %d", who, noun, index, lohi[k], ntypes);
  for (int k = 0; k < n; k += 2)
    if (lohi[k] > lohi[k + 1])
      return mdp_fail(c, MDP_EINVAL, "%s: %s %d: a type range with lo > hi (%d .. %d)", who, noun, index, lohi[k], lohi[k + 1]);
  return MDP_OK;
}

int mdp_measure_shell_setup(mdp_ctx *c, const char *who, const char *what, const char *whom, const double r)
{
  const double limit = mdp_measure_shell_limit(c);
  if (r > limit * (1.0 + 1e-12))
    return mdp_fail(c, MDP_EINVAL, "%s: %s %.15g + skin %g exceeds the ghost shell %.15g: only %s within %.15g are guaranteed present "
                                   "between two reneighbourings",
                    who, what, r, c->cfg.skin, c->dd.cutghost, whom, limit);
  return MDP_OK;
}

int mdp_measure_shell_read(mdp_ctx *c, const char *who, const char *what, const double r, const char *setup)
{
  const double limit = mdp_measure_shell_limit(c);
  if (r > limit * (1.0 + 1e-12))
    return mdp_fail(c, MDP_EINVAL, "%s: the %s %.15g of %s exceeds the current ghost shell less the skin, %.15g", who, what, r, setup, limit);
  return MDP_OK;
}

int mdp_measure_member(mdp_ctx *c, const char *who, const int ntag, const unsigned char *member_by_tag, DevBuf<unsigned char> &d_member,
                       int &ntag_kept)
{
  if (member_by_tag) {
    if (ntag < 1) return mdp_fail(c, MDP_EINVAL, "%s: a member table with ntag = %d", who, ntag);
    MDP_HIP(c, d_member.reserve((size_t) ntag + 8));
    MDP_TRY(mdp_host_upload(c, d_member.p, member_by_tag, (size_t) ntag));
    MDP_HIP(c, hipStreamSynchronize(c->stream)); // the caller's array may change after return
  }
  ntag_kept = member_by_tag ? ntag : 0;
  return MDP_OK;
}

int mdp_hist_open(mdp_ctx *c, const char *who, const char *what, const double r, const char *setup, unsigned long long *d_out,
                  const int nout)
{
  MDP_TRY(mdp_measure_shell_read(c, who, what, r, setup));
  MDP_TRY(mdp_md_flush_final(c));
  MDP_HIP(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * nout, c->stream));
  return MDP_OK;
}

int mdp_hist_download(mdp_ctx *c, const char *who, const char *setup, const unsigned long long *d_out, const int nout, const int ntag,
                      std::vector<unsigned long long> &host)
{
  host.resize((size_t) nout);
  MDP_TRY(mdp_read_one(c, d_out, sizeof(unsigned long long) * nout, host.data()));
  if (host[nout - 1])
    return mdp_fail(c, MDP_EINVAL, "%s: %lld owned or ghost atoms have a tag outside 1 .. %d, the member table of %s", who,
                    (long long) host[nout - 1], ntag, setup);
  return MDP_OK;
}

int mdp_measure_bin(mdp_ctx *c, MdpBinning &b, const double cutoff, const int ntypes, const int ntag,
                    const unsigned char *d_member, unsigned long long *d_bad, MdpGrid &g)
{
  hipStream_t st = c->stream;
  const int nall = c->nall;
  long long ncell;
  bin_grid(c, cutoff, g, ncell);
  MDP_HIP(c, b.key_a.reserve((size_t) nall + 1));
  MDP_HIP(c, b.key_b.reserve((size_t) nall + 1));
  MDP_HIP(c, b.val_a.reserve((size_t) nall + 1));
  MDP_HIP(c, b.perm.reserve((size_t) nall + 1));
  MDP_HIP(c, b.code.reserve((size_t) nall + 1));
  MDP_HIP(c, b.rec.reserve((size_t) nall + 1));
  MDP_HIP(c, b.cell_start.reserve((size_t) ncell + 2));
  bin_assign_kernel<<<nblk(nall), 256, 0, st>>>(g, nall, c->nlocal, ntypes, c->xq.p, c->type.p, c->tag.p, ntag, ntag ? d_member : nullptr,
                                                b.key_a.p, b.val_a.p, b.code.p, d_bad);
  MDP_HIP(c, hipGetLastError());
  int bits = 1;
  while ((1ll << bits) < ncell) bits++;
  size_t tmp = 0;
  MDP_HIP(c, rocprim::radix_sort_pairs(nullptr, tmp, b.key_a.p, b.key_b.p, b.val_a.p, b.perm.p, (size_t) nall, 0, bits, st));
  MDP_HIP(c, b.sort_tmp.reserve(tmp + 16));
  MDP_HIP(c, rocprim::radix_sort_pairs(b.sort_tmp.p, tmp, b.key_a.p, b.key_b.p, b.val_a.p, b.perm.p, (size_t) nall, 0, bits, st));
  bin_bounds_kernel<<<nblk(nall), 256, 0, st>>>(nall, b.key_b.p, b.perm.p, c->xq.p, b.code.p, b.cell_start.p, b.rec.p);
  bin_tail_kernel<<<1, 256, 0, st>>>(nall, (int) ncell, b.key_b.p, b.cell_start.p);
  MDP_HIP(c, hipGetLastError());
  return MDP_OK;
}
