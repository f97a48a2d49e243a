// coord.hip -- per-atom coordination numbers of a device-resident run (LAMMPS compute coord/atom cutoff), in integers.
// A read bins ALL atoms of the brick (owned and ghost) as a read of rdf.hip does (mdp_measure_bin, measure_bin.hip), without a
// member table -- partners of any group count -- at cell width >= cutoff / 2, into buffers that belong to MdpCoord.  Then one
// WAVE per centre at a time, four centres in flight per workgroup: the 64 lanes stride over the candidates of the centre's
// 5 x 5 stencil runs, laid end to end (the walk of adf.hip's phase A), test rsq < cutoff^2 and look up the candidate's column
// mask by its type; per batch of 64 candidates there is one ballot and one population count per column, and lane k keeps the
// counter of column k.  Lane k writes the centre's count of column k as a double into row perm[place] of the output, which
// is in the context's owned order.  A centre is an owned atom whose mask has the group bit; the rows of all other owned atoms
// stay 0.  Integers throughout and no atomic of any kind: two reads of one state agree exactly.
#include "mdp_common.h"

namespace {

constexpr int kCoordWaves = 4; // waves of a workgroup, each with the runs of its centre

using Grid = MdpGrid;

// the 25 runs of a centre's stencil: candidates in front of run k, and its first place
struct CoordRuns {
  int excl[32], base[32];
};

// the lanes of one wave have written LDS that other lanes of the same wave read next (or the reverse)
__device__ __forceinline__ void coord_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroups stride over the chunks of 256 places; within a chunk wave w takes the 64 places from 64 w, centre by centre.
// perm: place -> atom (an owned atom's index is its row of val and its entry of mask).
__global__ __launch_bounds__(256) void coord_count_kernel(const Grid g, const int nall, const int nchunk, const int ncol,
                                                          const int gbit, const double cutsq, const double4 *__restrict__ rec,
                                                          const int *__restrict__ cell_start, const int *__restrict__ perm,
                                                          const int *__restrict__ mask, const unsigned *__restrict__ tab_g,
                                                          double *__restrict__ val)
{
  __shared__ unsigned tab[kBinTypes];
  __shared__ CoordRuns runs[kCoordWaves];
  if (threadIdx.x < kBinTypes) tab[threadIdx.x] = tab_g[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  CoordRuns &L = runs[wave];
  for (int chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
    const int pi = chunk * 256 + threadIdx.x;
    int ai = -1; // the row of a centre; -1: a ghost, an atom outside the group, a place past the end
    double4 xi = make_double4(0.0, 0.0, 0.0, 0.0);
    if (pi < nall) {
      xi = rec[pi];
      if (__double2loint(xi.w) & kBinOwned) {
        ai = perm[pi];
        if (gbit && !(mask[ai] & gbit)) ai = -1;
      }
    }
    for (unsigned long long todo = __ballot(ai >= 0); todo; todo &= todo - 1) {
      const int src = __ffsll((long long) todo) - 1, pc = chunk * 256 + wave * 64 + src;
      double4 xc;
      xc.x = __shfl(xi.x, src, 64);
      xc.y = __shfl(xi.y, src, 64);
      xc.z = __shfl(xi.z, src, 64);
      const int ac = __shfl(ai, src, 64);
      int cx, cy, cz;
      mdp_bin_cell_index(g, xc, cx, cy, cz);
      const int x0 = max(cx - 2, 0), x1 = min(cx + 2, g.n[0] - 1);
      // the 25 runs of the stencil (cells along x are contiguous in the sort), one per lane, then a prefix sum of their lengths
      int len = 0, pb = 0;
      if (lane < 25) {
        const int z = cz - 2 + lane / 5, y = cy - 2 + lane % 5;
        if (z >= 0 && z < g.n[2] && y >= 0 && y < g.n[1]) {
          const int c0 = g.n[0] * (y + g.n[1] * z);
          pb = cell_start[c0 + x0];
          len = cell_start[c0 + x1 + 1] - pb;
        }
      }
      int incl = len;
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      if (lane < 32) {
        L.excl[lane] = incl - len;
        L.base[lane] = pb;
      }
      const int total = __shfl(incl, 31, 64); // (lanes 25 .. 31 add nothing)
      coord_wave_sync();
      unsigned cnt = 0u; // lane k: the centre's count of column k
      for (int q0 = 0; q0 < total; q0 += 64) {
        const int q = q0 + lane;
        unsigned m = 0u;
        if (q < total) {
          int r = 0; // the last run that starts at or before q: the one that holds it
#pragma unroll
          for (int k = 1; k < 25; k++) r += q >= L.excl[k];
          const int p = L.base[r] + (q - L.excl[r]);
          const double4 xj = rec[p];
          const double dx = xj.x - xc.x, dy = xj.y - xc.y, dz = xj.z - xc.z;
          const double rsq = dx * dx + dy * dy + dz * dz;
          if (rsq < cutsq && p != pc) m = tab[__double2loint(xj.w) & (kBinTypes - 1)];
        }
        for (int k = 0; k < ncol; k++) {
          const unsigned long long bal = __ballot((m >> k) & 1u);
          if (lane == k) cnt += (unsigned) __popcll(bal);
        }
      }
      if (lane < ncol) val[(size_t) ac * ncol + lane] = (double) cnt;
      coord_wave_sync(); // the runs are free for the wave's next centre
    }
  }
}

} // namespace

void mdp_coord_release(mdp_ctx *c)
{
  MdpCoord &h = c->coord;
  h.tab.release();
  h.bin.release();
  h.val.release();
  h.on = false;
}

extern "C" {

int mdp_coord_setup(mdp_ctx *c, double cutoff, int ncol, const int *jlo, const int *jhi, int groupbit)
{
  MDP_TRY(mdp_measure_require(c, "mdp_coord_setup"));
  if (ncol < 1 || ncol > MDP_COORD_MAXCOL)
    return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: ncol must be 1 .. %d, not %d", MDP_COORD_MAXCOL, ncol);
  if (!jlo || !jhi) return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: no type ranges");
  // (1 .. 15 atom types: see mdp_rdf_setup)
  const int ntypes = c->ntypes > 0 ? c->ntypes : c->cfg.ntypes;
  if (ntypes < 1 || ntypes >= kBinTypes)
    return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: %d atom types (the type code of a record holds 1 .. %d)", ntypes, kBinTypes - 1);
  for (int m = 0; m < ncol; m++) {
    if (jlo[m] < 1 || jlo[m] > ntypes || jhi[m] < 1 || jhi[m] > ntypes)
      return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: column %d: type %d outside 1 .. %d", m + 1,
                      jlo[m] < 1 || jlo[m] > ntypes ? jlo[m] : jhi[m], ntypes);
    if (jlo[m] > jhi[m]) return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: column %d: a type range with lo > hi (%d .. %d)", m + 1, jlo[m], jhi[m]);
  }
  if (!(cutoff > 0.0) || !std::isfinite(cutoff)) return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: cutoff must be > 0, not %g", cutoff);
  // the ghost shell and the skin: the argument of mdp_rdf_setup
  const double limit = c->dd.cutghost - c->cfg.skin;
  if (cutoff > limit * (1.0 + 1e-12))
    return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: cutoff %.15g + skin %g exceeds the ghost shell %.15g: only partners within %.15g are "
                                   "guaranteed present between two reneighbourings",
                    cutoff, c->cfg.skin, c->dd.cutghost, limit);
  MDP_TRY(mdp_require_group_mask(c, "mdp_coord_setup", groupbit, false));
  MdpCoord &h = c->coord;
  unsigned tab[kBinTypes] = {};
  for (int m = 0; m < ncol; m++)
    for (int t = jlo[m]; t <= jhi[m]; t++) tab[t] |= 1u << m;
  MDP_HIP(c, h.tab.reserve(kBinTypes));
  MDP_TRY(mdp_write_small(c, h.tab.p, tab, sizeof tab));
  h.ncol = ncol;
  h.ntypes = ntypes;
  h.gbit = groupbit;
  h.cutoff = cutoff;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_coord_read(mdp_ctx *c, int *tag, double *values)
{
  MDP_TRY(mdp_measure_require(c, "mdp_coord_read"));
  if (!tag || !values) return MDP_EINVAL;
  MdpCoord &h = c->coord;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_coord_setup not called");
  MDP_TRY(mdp_peratom_open(c, "mdp_coord_read", h.cutoff, h.gbit));
  hipStream_t st = c->stream;
  const int nall = c->nall, nlocal = c->nlocal;
  if (nall > 0 && nlocal > 0) {
    MDP_HIP(c, h.val.reserve((size_t) nlocal * h.ncol + 1));
    MDP_HIP(c, hipMemsetAsync(h.val.p, 0, sizeof(double) * (size_t) nlocal * h.ncol, st));
    Grid g;
    // (no member table: the counter of bad tags is never written; the output's spare word stands in for it)
    MDP_TRY(mdp_measure_bin(c, h.bin, h.cutoff, h.ntypes, 0, nullptr, (unsigned long long *) (h.val.p + (size_t) nlocal * h.ncol), g));
    const int nchunk = nblk(nall);
    if (c->num_cu <= 0) {
      int n = 0;
      MDP_HIP(c, hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device));
      c->num_cu = n > 0 ? n : 256;
    }
    const int grid = mdp_measure_grid(nchunk, 8 * c->num_cu); // 8 workgroups of 4 waves fill a CU; LDS is no limit here
    MDP_TRY(mdp_launch(c, coord_count_kernel, grid, 256, 0, st, g, nall, nchunk, h.ncol, h.gbit, h.cutoff * h.cutoff, h.bin.rec.p,
                       h.bin.cell_start.p, h.bin.perm.p, h.gbit ? c->mask.p : nullptr, h.tab.p, h.val.p));
  }
  return mdp_peratom_download(c, h.val.p, h.ncol, tag, values);
}

int mdp_coord_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->coord, c->coord.ncol, c->coord.gbit, out);
}

int mdp_coord_off(mdp_ctx *c) { return mdp_measure_off(c, mdp_coord_release); }

} // extern "C"
