// cna.hip -- the per-atom common neighbour analysis of a device-resident run (LAMMPS compute cna/atom Rc): 1 fcc, 2 hcp, 3 bcc,
// 4 icosahedral, 5 other, 0 outside the group.
// A read bins ALL atoms of the brick (owned and ghost) as a read of rdf.hip does (mdp_measure_bin, measure_bin.hip), without a
// member table -- neighbours of any group count -- at cell width >= cutoff / 2, into buffers that belong to MdpCna.  Then one
// WAVE per centre at a time, four centres in flight per workgroup:
//   gather     the 64 lanes stride over the candidates of the centre's 5 x 5 stencil runs, laid end to end, test rsq < cutoff^2
//              and compact the hits by ballot and prefix count into the wave's short list in LDS {dx, dy, dz}, MDP_CNA_MAXNEAR
//              entries, in the order of their places (the walk of measure_walk.h).  A hit past the list's end
//              is counted, not stored: a centre with n neighbours, n not 12 or 14, is `other` whatever n is;
//   adjacency  lane (a = lane & 15, quarter = lane >> 4) tests entry a against the entries 4 quarter .. 4 quarter + 3 -- the
//              distance between two neighbours is formed from the difference of their displacements -- and two cross-lane
//              ORs leave the row mask adj[a], bit k: entries a and k are closer than the cutoff, in every lane with lane & 15 = a;
//   signature  any common neighbour of the centre and its neighbour m is a neighbour of the centre, so `common` of bond m is
//              adj[m]: lane m < n has ncommon = popc(adj[m]) and, for every set bit k with adj[k] by shuffle, the bonds of k
//              inside common, popc(adj[k] & adj[m]): their sum is 2 nbonds, their maximum maxbond, their minimum (from 8, as
//              LAMMPS initialises it) minbond;
//   pattern    one ballot per signature the patterns ask for, a population count each, and lane 0 stores the pattern as a
//              double.  Lane p of a wave counts its centres of pattern p and lane 6 those with more than MDP_CNA_MAXNEAR
//              neighbours; a wave adds its counters to the global ones once, at its end, as 64-bit integers.
// Every lane runs every trip and every shuffle: n is the same in all lanes of a wave, and so is every branch on it.  Integers
// throughout and no floating-point atomic anywhere: two reads of one state agree bit for bit.
#include "measure_walk.h"

namespace {

constexpr int kCnaWaves = 4; // waves of a workgroup, each with a short list of its own
constexpr int kCnaMinbond0 = 8; // minbond of an empty set of common neighbours: LAMMPS' MAXCOMMON

using Grid = MdpGrid;

// a wave's LDS: the centre's first MDP_CNA_MAXNEAR neighbours inside the cutoff and the 25 runs of its stencil: 640 bytes
struct CnaList {
  double dx[MDP_CNA_MAXNEAR], dy[MDP_CNA_MAXNEAR], dz[MDP_CNA_MAXNEAR];
  MdpWalkRuns runs;
};

// Workgroups stride over the chunks of 256 places; within a chunk wave w takes the 64 places from 64 w, centre by centre.
// perm: place -> atom (an owned atom's index is its entry of val and of mask).  cnt[0 .. 5]: centres per pattern, cnt[6]: centres
// with more than MDP_CNA_MAXNEAR neighbours.
__global__ __launch_bounds__(256) void cna_kernel(const Grid g, const int nall, const int nchunk, const int gbit, const double cutsq,
                                                  const double4 *__restrict__ rec, const int *__restrict__ cell_start,
                                                  const int *__restrict__ perm, const int *__restrict__ mask,
                                                  double *__restrict__ val, unsigned long long *__restrict__ cnt)
{
  static_assert(MDP_CNA_MAXNEAR == 16, "a row of the adjacency is one 16-bit mask, four columns per quarter of the wave");
  __shared__ CnaList lists[kCnaWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = lane & 15, c0 = (lane >> 4) * 4;
  CnaList &L = lists[wave];
  unsigned tally = 0u; // lane p < 6: the wave's centres of pattern p; lane 6: those over the cap
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
        if (hit && at < MDP_CNA_MAXNEAR) {
          L.dx[at] = c.dx;
          L.dy[at] = c.dy;
          L.dz[at] = c.dz;
        }
      }
      mdp_wave_sync();
      int pattern = 5;
      if (n == 12 || n == 14) {
        // ---- adjacency: row a against the columns c0 .. c0 + 3
        unsigned adj = 0u;
        if (a < n) {
          const double ax = L.dx[a], ay = L.dy[a], az = L.dz[a];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int b = c0 + k;
            if (b < n && b != a) {
              const double ux = L.dx[b] - ax, uy = L.dy[b] - ay, uz = L.dz[b] - az;
              if (ux * ux + uy * uy + uz * uz < cutsq) adj |= 1u << b;
            }
          }
        }
        adj |= (unsigned) __shfl_xor((int) adj, 16, 64);
        adj |= (unsigned) __shfl_xor((int) adj, 32, 64);
        // ---- signature of bond `lane` (lanes 0 .. 15 hold the rows 0 .. 15; a row past n is empty)
        int twice = 0, maxbond = 0, minbond = kCnaMinbond0;
        for (int k = 0; k < n; k++) {
          const unsigned row = (unsigned) __shfl((int) adj, k, 64);
          if ((adj >> k) & 1u) {
            const int b = __popc(row & adj);
            twice += b;
            maxbond = max(maxbond, b);
            minbond = min(minbond, b);
          }
        }
        const int ncommon = __popc(adj), nbonds = twice / 2;
        const bool bond = lane < n;
        const auto votes = [&](const int cj, const int ck, const int cl, const int cm) {
          return __popcll(__ballot(bond && ncommon == cj && nbonds == ck && maxbond == cl && minbond == cm));
        };
        if (n == 12) {
          const int nfcc = votes(4, 2, 1, 1), nhcp = votes(4, 2, 2, 0), nico = votes(5, 5, 2, 2);
          if (nfcc == 12) pattern = 1;
          else if (nfcc == 6 && nhcp == 6) pattern = 2;
          else if (nico == 12) pattern = 4;
        } else {
          const int nbcc4 = votes(4, 4, 2, 2), nbcc6 = votes(6, 6, 2, 2);
          if (nbcc4 == 6 && nbcc6 == 8) pattern = 3;
        }
      }
      if (lane == 0) val[ctr.v] = (double) pattern;
      tally += (lane == pattern) || (lane == 6 && n > MDP_CNA_MAXNEAR);
      mdp_wave_sync(); // the list is free for the wave's next centre
    }
  }
  if (lane < 7 && tally) atomicAdd(cnt + lane, (unsigned long long) tally);
}

} // namespace

static void cna_release(mdp_ctx *c) // mdp_cna_off: the measurement's buffers go ahead of the context's end
{
  MdpCna &h = c->cna;
  h.bin.release();
  h.val.release();
  h.cnt.release();
  h.on = false;
  h.over = 0;
  for (int p = 0; p < 6; p++) h.counts[p] = 0;
}

extern "C" {

int mdp_cna_setup(mdp_ctx *c, double cutoff, int groupbit)
{
  MDP_TRY(mdp_measure_require(c, "mdp_cna_setup"));
  int ntypes;
  MDP_TRY(mdp_measure_ntypes(c, "mdp_cna_setup", ntypes));
  if (!(cutoff > 0.0) || !std::isfinite(cutoff)) return mdp_fail(c, MDP_EINVAL, "mdp_cna_setup: cutoff must be > 0, not %g", cutoff);
  MDP_TRY(mdp_measure_shell_setup(c, "mdp_cna_setup", "cutoff", "neighbours", cutoff));
  MDP_TRY(mdp_require_group_mask(c, "mdp_cna_setup", groupbit, false));
  MdpCna &h = c->cna;
  MDP_HIP(c, h.cnt.reserve(8));
  h.ntypes = ntypes;
  h.gbit = groupbit;
  h.cutoff = cutoff;
  h.over = 0;
  for (int p = 0; p < 6; p++) h.counts[p] = 0;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_cna_read(mdp_ctx *c, int *tag, double *values)
{
  MDP_TRY(mdp_measure_require(c, "mdp_cna_read"));
  if (!tag || !values) return MDP_EINVAL;
  MdpCna &h = c->cna;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_cna_setup not called");
  MDP_TRY(mdp_peratom_open(c, "mdp_cna_read", h.cutoff, h.gbit));
  hipStream_t st = c->stream;
  const int nall = c->nall, nlocal = c->nlocal;
  MDP_HIP(c, hipMemsetAsync(h.cnt.p, 0, sizeof(unsigned long long) * 8, st));
  if (nall > 0 && nlocal > 0) {
    MDP_HIP(c, h.val.reserve((size_t) nlocal + 1));
    MDP_HIP(c, hipMemsetAsync(h.val.p, 0, sizeof(double) * (size_t) nlocal, st));
    Grid g;
    MDP_TRY(mdp_measure_bin(c, h.bin, h.cutoff, h.ntypes, 0, nullptr, h.cnt.p + 7, g)); // (no member table: cnt[7] is never written)
    const int nchunk = nblk(nall);
    int resident;
    MDP_TRY(mdp_measure_resident(c, sizeof(CnaList) * kCnaWaves, resident)); // (2.5 KB a workgroup: LDS is no limit here)
    const int grid = mdp_measure_grid(nchunk, resident);
    MDP_TRY(mdp_launch(c, cna_kernel, grid, 256, 0, st, g, nall, nchunk, h.gbit, h.cutoff * h.cutoff, h.bin.rec.p, h.bin.cell_start.p,
                       h.bin.perm.p, h.gbit ? c->mask.p : nullptr, h.val.p, h.cnt.p));
  }
  unsigned long long cnt[7] = {0, 0, 0, 0, 0, 0, 0};
  MDP_TRY(mdp_read_one(c, h.cnt.p, sizeof cnt, cnt));
  for (int p = 0; p < 6; p++) h.counts[p] = (long long) cnt[p];
  h.over = (long long) cnt[6];
  return mdp_peratom_download(c, h.val.p, 1, tag, values);
}

int mdp_cna_counts(mdp_ctx *c, long long out[6])
{
  if (!c || !out) return MDP_EINVAL;
  if (!c->cna.on) return mdp_fail(c, MDP_ESTATE, "mdp_cna_setup not called");
  for (int p = 0; p < 6; p++) out[p] = c->cna.counts[p];
  return MDP_OK;
}

int mdp_cna_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->cna, 0, c->cna.over, out);
}

int mdp_cna_off(mdp_ctx *c) { return mdp_measure_off(c, cna_release); }

} // extern "C"
