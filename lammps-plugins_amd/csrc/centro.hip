// centro.hip -- the per-atom centro-symmetry parameter of a device-resident run (LAMMPS compute centro/atom without axes).
// A read bins ALL atoms of the brick (owned and ghost) as a read of rdf.hip does (mdp_measure_bin, measure_bin.hip), without a
// member table -- partners of any group count -- at cell width >= cutoff / 2, into buffers that belong to MdpCentro.  Then one
// WAVE per centre at a time, four centres in flight per workgroup:
//   gather  the 64 lanes stride over the candidates of the centre's 5 x 5 stencil runs, laid end to end, test rsq < cutoff^2 and
//           compact the hits by ballot and prefix count into the wave's short list in LDS {dx, dy, dz, rsq}, MDP_ADF_MAXNEIGH
//           entries, in the order of their places (the walk of measure_walk.h, which adf.hip and coord.hip share);
//   select  the rank of an entry is the number of entries with a smaller (rsq, list index) -- the list is in place order, so a tie
//           breaks on the place and never on lane timing --; the entries of rank < N go to slot [rank] of a second list;
//   sum     the lanes stride over the N (N - 1) / 2 pairs a < b of that list and write |R_a + R_b|^2 to LDS; the rank of a
//           value is counted the same way over (value, pair index), the values of rank < N / 2 go to slot [rank], and lane 0
//           adds them in ascending order.
// A centre with more hits than the short list holds is counted, not truncated, and the read is refused; one with fewer than N
// gets 0 and is counted.  No floating-point atomic anywhere: two reads of one state agree bit for bit.
#include "measure_walk.h"

namespace {

constexpr int kCentroWaves = 4; // waves of a workgroup, each with a short list of its own

using Grid = MdpGrid;

// the fixed part of a wave's LDS: the centre's neighbours inside the cutoff and the 25 runs of its stencil
struct CentroList {
  double dx[MDP_ADF_MAXNEIGH], dy[MDP_ADF_MAXNEIGH], dz[MDP_ADF_MAXNEIGH], rsq[MDP_ADF_MAXNEIGH];
  MdpWalkRuns runs;
};
// ... and the part that grows with N, in doubles: the N nearest {x, y, z}, the pair values, the N / 2 smallest of them
__host__ __device__ constexpr int centro_npair(const int nnn) { return nnn * (nnn - 1) / 2; }
__host__ __device__ constexpr int centro_wave_doubles(const int nnn) { return 3 * nnn + centro_npair(nnn) + nnn / 2; }
// LDS of a workgroup in bytes: 4.3 KB + 8 (3 N + N (N - 1) / 2 + N / 2) per wave: 20 KB at N = 12, 88 KB at N = 64
size_t centro_lds_bytes(const int nnn) { return kCentroWaves * (sizeof(CentroList) + sizeof(double) * centro_wave_doubles(nnn)); }

// Workgroups stride over the chunks of 256 places; within a chunk wave w takes the 64 places from 64 w, centre by centre.
// perm: place -> atom (an owned atom's index is its entry of val and of mask).  cnt[0]: centres over the cap, cnt[1]: centres
// with fewer than nnn partners.
__global__ __launch_bounds__(256) void centro_kernel(const Grid g, const int nall, const int nchunk, const int nnn, const int gbit,
                                                     const double cutsq, const double4 *__restrict__ rec,
                                                     const int *__restrict__ cell_start, const int *__restrict__ perm,
                                                     const int *__restrict__ mask, double *__restrict__ val,
                                                     unsigned long long *__restrict__ cnt)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char centro_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npair = centro_npair(nnn), half = nnn / 2;
  CentroList &L = ((CentroList *) centro_lds)[wave];
  double *sx = (double *) (centro_lds + kCentroWaves * sizeof(CentroList)) + (size_t) wave * centro_wave_doubles(nnn);
  double *sy = sx + nnn, *sz = sy + nnn, *pv = sz + nnn, *sm = pv + npair;
  for (int chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
    const int pi = chunk * 256 + threadIdx.x;
    int ai = -1; // the entry of a centre; -1: a ghost, an atom outside the group, a place past the end
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
      // ---- gather
      const int total = mdp_walk_runs(g, cell_start, ctr.x, lane, L.runs);
      int n = 0; // hits so far: the same in every lane
      for (int q0 = 0; q0 < total; q0 += 64) {
        MdpWalkCand c;
        const bool has = mdp_walk_cand(L.runs, q0 + lane, total, rec, ctr.x, c);
        const bool hit = has && c.rsq < cutsq && c.p != ctr.p;
        const int at = mdp_walk_slot(hit, lane, n);
        if (hit && at < MDP_ADF_MAXNEIGH) {
          L.dx[at] = c.dx;
          L.dy[at] = c.dy;
          L.dz[at] = c.dz;
          L.rsq[at] = c.rsq;
        }
      }
      mdp_wave_sync();
      if (n > MDP_ADF_MAXNEIGH) {
        if (lane == 0) atomicAdd(cnt, 1ull);
      } else if (n < nnn) {
        if (lane == 0) atomicAdd(cnt + 1, 1ull); // (its value stays 0)
      } else {
        // ---- select: the nnn nearest, into slot [rank]
        for (int e = lane; e < n; e += 64) {
          const double r = L.rsq[e];
          int rank = 0;
          for (int k = 0; k < n; k++) {
            const double rk = L.rsq[k];
            rank += (rk < r) || (rk == r && k < e);
          }
          if (rank < nnn) {
            sx[rank] = L.dx[e];
            sy[rank] = L.dy[e];
            sz[rank] = L.dz[e];
          }
        }
        mdp_wave_sync();
        // ---- sum: pair q is (a, b), a < b, row by row: q = a (nnn - 1) - a (a - 1) / 2 + (b - a - 1)
        for (int q = lane; q < npair; q += 64) {
          int a = 0, rem = q;
          while (rem >= nnn - 1 - a) {
            rem -= nnn - 1 - a;
            a++;
          }
          const int b = a + 1 + rem;
          const double ux = sx[a] + sx[b], uy = sy[a] + sy[b], uz = sz[a] + sz[b];
          pv[q] = ux * ux + uy * uy + uz * uz;
        }
        mdp_wave_sync();
        for (int q = lane; q < npair; q += 64) {
          const double v = pv[q];
          int rank = 0;
          for (int k = 0; k < npair; k++) {
            const double vk = pv[k];
            rank += (vk < v) || (vk == v && k < q);
          }
          if (rank < half) sm[rank] = v;
        }
        mdp_wave_sync();
        if (lane == 0) {
          double s = 0.0;
          for (int k = 0; k < half; k++) s += sm[k];
          val[ctr.v] = s;
        }
      }
      mdp_wave_sync(); // the lists are free for the wave's next centre
    }
  }
}

} // namespace

static void centro_release(mdp_ctx *c) // mdp_centro_off: the measurement's buffers go ahead of the context's end
{
  MdpCentro &h = c->centro;
  h.bin.release();
  h.val.release();
  h.cnt.release();
  h.on = false;
  h.few = 0;
}

extern "C" {

int mdp_centro_setup(mdp_ctx *c, int nnn, double cutoff, int groupbit)
{
  MDP_TRY(mdp_measure_require(c, "mdp_centro_setup"));
  if (nnn < 2 || nnn > MDP_CENTRO_MAXN)
    return mdp_fail(c, MDP_EINVAL, "mdp_centro_setup: the number of neighbours must be 2 .. %d (the pair values of a wave in LDS), not %d",
                    MDP_CENTRO_MAXN, nnn);
  if (nnn % 2) return mdp_fail(c, MDP_EINVAL, "mdp_centro_setup: the number of neighbours must be even, not %d", nnn);
  int ntypes;
  MDP_TRY(mdp_measure_ntypes(c, "mdp_centro_setup", ntypes));
  if (!std::isfinite(cutoff)) return mdp_fail(c, MDP_EINVAL, "mdp_centro_setup: cutoff %g", cutoff);
  if (!(cutoff > 0.0)) cutoff = mdp_measure_shell_limit(c); // the default: all that the ghost shell guarantees
  if (!(cutoff > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_centro_setup: the ghost shell %.15g less the skin %g leaves no cutoff", c->dd.cutghost, c->cfg.skin);
  MDP_TRY(mdp_measure_shell_setup(c, "mdp_centro_setup", "cutoff", "partners", cutoff));
  MDP_TRY(mdp_require_group_mask(c, "mdp_centro_setup", groupbit, false));
  MdpCentro &h = c->centro;
  MDP_HIP(c, h.cnt.reserve(4));
  h.nnn = nnn;
  h.ntypes = ntypes;
  h.gbit = groupbit;
  h.cutoff = cutoff;
  h.few = 0;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_centro_read(mdp_ctx *c, int *tag, double *values)
{
  MDP_TRY(mdp_measure_require(c, "mdp_centro_read"));
  if (!tag || !values) return MDP_EINVAL;
  MdpCentro &h = c->centro;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_centro_setup not called");
  MDP_TRY(mdp_peratom_open(c, "mdp_centro_read", h.cutoff, h.gbit));
  hipStream_t st = c->stream;
  const int nall = c->nall, nlocal = c->nlocal;
  MDP_HIP(c, hipMemsetAsync(h.cnt.p, 0, sizeof(unsigned long long) * 4, st));
  if (nall > 0 && nlocal > 0) {
    MDP_HIP(c, h.val.reserve((size_t) nlocal + 1));
    MDP_HIP(c, hipMemsetAsync(h.val.p, 0, sizeof(double) * (size_t) nlocal, st));
    Grid g;
    MDP_TRY(mdp_measure_bin(c, h.bin, h.cutoff, h.ntypes, 0, nullptr, h.cnt.p + 2, g)); // (no member table: cnt[2] is never written)
    const int nchunk = nblk(nall);
    const size_t lds = centro_lds_bytes(h.nnn);
    int resident;
    MDP_TRY(mdp_measure_resident(c, lds, resident));
    const int grid = mdp_measure_grid(nchunk, resident);
    MDP_TRY(mdp_launch(c, centro_kernel, grid, 256, lds, st, g, nall, nchunk, h.nnn, h.gbit, h.cutoff * h.cutoff, h.bin.rec.p,
                       h.bin.cell_start.p, h.bin.perm.p, h.gbit ? c->mask.p : nullptr, h.val.p, h.cnt.p));
  }
  unsigned long long cnt[2] = {0, 0};
  MDP_TRY(mdp_read_one(c, h.cnt.p, sizeof cnt, cnt));
  if (cnt[0])
    return mdp_fail(c, MDP_EINVAL, "mdp_centro_read: %lld centres have more than %d atoms inside the cutoff %g, the short list of a wave: "
                                   "use a smaller cutoff",
                    (long long) cnt[0], MDP_ADF_MAXNEIGH, h.cutoff);
  h.few = (long long) cnt[1];
  return mdp_peratom_download(c, h.val.p, 1, tag, values);
}

int mdp_centro_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->centro, c->centro.nnn, c->centro.few, out);
}

int mdp_centro_off(mdp_ctx *c) { return mdp_measure_off(c, centro_release); }

} // extern "C"
