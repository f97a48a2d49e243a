// coord.hip -- per-atom coordination numbers of a device-resident run (LAMMPS compute coord/atom cutoff), in integers.
// A read bins ALL atoms of the brick (owned and ghost) as a read of rdf.hip does (mdp_measure_bin, measure_bin.hip), without a
// member table -- partners of any group count -- at cell width >= cutoff / 2, into buffers that belong to MdpCoord.  Then one
// WAVE per centre at a time, four centres in flight per workgroup: the 64 lanes stride over the candidates of the centre's
// 5 x 5 stencil runs, laid end to end (the walk of measure_walk.h), test rsq < cutoff^2 and look up the candidate's column
// mask by its type; per batch of 64 candidates there is one ballot and one population count per column, and lane k keeps the
// counter of column k.  Lane k writes the centre's count of column k as a double into row perm[place] of the output, which
// is in the context's owned order.  A centre is an owned atom whose mask has the group bit; the rows of all other owned atoms
// stay 0.  Integers throughout and no atomic of any kind: two reads of one state agree exactly.
#include "measure_walk.h"

namespace {

constexpr int kCoordWaves = 4; // waves of a workgroup, each with the runs of its centre

using Grid = MdpGrid;

// Workgroups stride over the chunks of 256 places; within a chunk wave w takes the 64 places from 64 w, centre by centre.
// perm: place -> atom (an owned atom's index is its row of val and its entry of mask).
__global__ __launch_bounds__(256) void coord_count_kernel(const Grid g, const int nall, const int nchunk, const int ncol,
                                                          const int gbit, const double cutsq, const double4 *__restrict__ rec,
                                                          const int *__restrict__ cell_start, const int *__restrict__ perm,
                                                          const int *__restrict__ mask, const unsigned *__restrict__ tab_g,
                                                          double *__restrict__ val)
{
  __shared__ unsigned tab[kBinTypes];
  __shared__ MdpWalkRuns runs[kCoordWaves];
  if (threadIdx.x < kBinTypes) tab[threadIdx.x] = tab_g[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  MdpWalkRuns &L = runs[wave];
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
      const MdpWalkCentre ctr = mdp_walk_centre(todo, xi, ai, chunk * 256 + wave * 64);
      const int total = mdp_walk_runs(g, cell_start, ctr.x, lane, L);
      unsigned cnt = 0u; // lane k: the centre's count of column k
      for (int q0 = 0; q0 < total; q0 += 64) {
        MdpWalkCand c;
        const bool has = mdp_walk_cand(L, q0 + lane, total, rec, ctr.x, c);
        const unsigned m = has && c.rsq < cutsq && c.p != ctr.p ? tab[__double2loint(c.xj.w) & (kBinTypes - 1)] : 0u;
        for (int k = 0; k < ncol; k++) {
          const unsigned long long bal = __ballot((m >> k) & 1u);
          if (lane == k) cnt += (unsigned) __popcll(bal);
        }
      }
      if (lane < ncol) val[(size_t) ctr.v * ncol + lane] = (double) cnt;
      mdp_wave_sync(); // the runs are free for the wave's next centre
    }
  }
}

} // namespace

static void coord_release(mdp_ctx *c) // mdp_coord_off: the measurement's buffers go ahead of the context's end
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
  int ntypes;
  MDP_TRY(mdp_measure_ntypes(c, "mdp_coord_setup", ntypes));
  for (int m = 0; m < ncol; m++) {
    const int r[2] = {jlo[m], jhi[m]};
    MDP_TRY(mdp_measure_type_ranges(c, "mdp_coord_setup", "column", m + 1, ntypes, 2, r));
  }
  if (!(cutoff > 0.0) || !std::isfinite(cutoff)) return mdp_fail(c, MDP_EINVAL, "mdp_coord_setup: cutoff must be > 0, not %g", cutoff);
  MDP_TRY(mdp_measure_shell_setup(c, "mdp_coord_setup", "cutoff", "partners", cutoff));
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
    int resident;
    MDP_TRY(mdp_measure_resident(c, sizeof(MdpWalkRuns) * kCoordWaves, resident)); // (8 workgroups of 4 waves fill a CU; LDS is no limit here)
    const int grid = mdp_measure_grid(nchunk, resident);
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

int mdp_coord_off(mdp_ctx *c) { return mdp_measure_off(c, coord_release); }

} // extern "C"
