// measure_walk.h -- what the wave-per-centre measurement kernels share on the device (adf.hip, coord.hip, centro.hip; rdf.hip takes
// the flush alone): a wave takes the centres among its 64 places one by one (mdp_walk_centre), lays the 25 runs of a centre's
// 5 x 5 x 5 stencil end to end (mdp_walk_runs) and strides over the candidates, 64 per trip (mdp_walk_cand);
// hits are compacted into a short list by ballot (mdp_walk_slot).  DESIGN.md section 4 item 46.  Device code only.
#pragma once
#include "mdp_common.h"

// the lanes of one wave have written LDS that other lanes of the same wave read next (or the reverse)
__device__ __forceinline__ void mdp_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// adds the workgroup's non-zero LDS counters to the global ones and clears them; every lane of the workgroup (256) calls it
__device__ __forceinline__ void mdp_lds_flush(unsigned *lds, const int n, unsigned long long *__restrict__ glob)
{
  __syncthreads();
  for (int k = threadIdx.x; k < n; k += 256) {
    const unsigned v = lds[k];
    if (v) {
      atomicAdd(glob + k, (unsigned long long) v);
      lds[k] = 0u;
    }
  }
  __syncthreads();
}

// The head of the centre loop.  A wave takes the centres among its 64 places one by one,
//   for (unsigned long long todo = __ballot(is_centre); todo; todo &= todo - 1) { const MdpWalkCentre ctr = mdp_walk_centre(todo, xi, v, p0); ...
// and this hands every lane the next one: its record (x, y, z), its place and the integer v of the lane that holds it.
// p0: the place of the wave's lane 0.
struct MdpWalkCentre {
  double4 x;
  int p, v;
};
__device__ __forceinline__ MdpWalkCentre mdp_walk_centre(const unsigned long long todo, const double4 &xi, const int v, const int p0)
{
  const int src = __ffsll((long long) todo) - 1;
  MdpWalkCentre ctr;
  ctr.x.x = __shfl(xi.x, src, 64);
  ctr.x.y = __shfl(xi.y, src, 64);
  ctr.x.z = __shfl(xi.z, src, 64);
  ctr.x.w = 0.0;
  ctr.p = p0 + src;
  ctr.v = __shfl(v, src, 64);
  return ctr;
}

// the 25 runs of a centre's stencil, in a wave's LDS: candidates in front of run k, and its first place
struct MdpWalkRuns {
  int excl[32], base[32];
};

// Fills the table for the centre at xc and returns the number of candidates.  The 25 runs (cells along x are contiguous in the
// sort), one per lane: their bounds in one round trip and not in 25, then a prefix sum of their lengths, so that the lanes
// can stride over the runs laid end to end.  Ends with the wave's sync: every lane may read the table.
__device__ __forceinline__ int mdp_walk_runs(const MdpGrid &g, const int *__restrict__ cell_start, const double4 &xc, const int lane,
                                             MdpWalkRuns &L)
{
  int cx, cy, cz;
  mdp_bin_cell_index(g, xc, cx, cy, cz);
  const int x0 = max(cx - 2, 0), x1 = min(cx + 2, g.n[0] - 1);
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
  mdp_wave_sync();
  return total;
}

// a candidate of a centre: its place, its record and where it lies from the centre
struct MdpWalkCand {
  int p;
  double4 xj;
  double dx, dy, dz, rsq;
};

// The 64 lanes stride over the `total` candidates of the table, 64 per trip:
//   for (int q0 = 0; q0 < total; q0 += 64) { MdpWalkCand c; const bool has = mdp_walk_cand(L, q0 + lane, total, rec, xc, c); ...
// EVERY lane runs the rest of the trip (the callers ballot in it); has: candidate q exists, and c is this lane's.  Without one
// c.p is -1 and the rest 0.  The centre itself is among the candidates: c.p != its place is the caller's to ask.
__device__ __forceinline__ bool mdp_walk_cand(const MdpWalkRuns &L, const int q, const int total, const double4 *__restrict__ rec,
                                              const double4 &xc, MdpWalkCand &c)
{
  c = MdpWalkCand{-1, make_double4(0.0, 0.0, 0.0, 0.0), 0.0, 0.0, 0.0, 0.0};
  if (q < total) {
    int r = 0; // the last run that starts at or before q: the one that holds it (an empty run starts where the next does)
#pragma unroll
    for (int k = 1; k < 25; k++) r += q >= L.excl[k];
    c.p = L.base[r] + (q - L.excl[r]);
    c.xj = rec[c.p];
    c.dx = c.xj.x - xc.x;
    c.dy = c.xj.y - xc.y;
    c.dz = c.xj.z - xc.z;
    c.rsq = c.dx * c.dx + c.dy * c.dy + c.dz * c.dz;
  }
  return q < total;
}

// A hit's slot in a short list that holds n entries so far, by ballot and prefix count; n, the same in every lane, moves on by
// the hits of the wave.  A slot may lie past the list's end: the caller stores below its cap and compares n with it after the walk.
__device__ __forceinline__ int mdp_walk_slot(const bool hit, const int lane, int &n)
{
  const unsigned long long bal = __ballot(hit);
  const int at = n + __popcll(bal & ((1ull << lane) - 1ull));
  n += __popcll(bal);
  return at;
}
