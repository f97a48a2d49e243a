// tiles.hip -- the tile-row layer both pair styles walk: the 16-row tiles, their unions (tu / tile_nu), the 16-bit
// rows (lj16) and the pruned copy of them (lj16_in / lj_len_in / lj_split_in).  Built from the bin grid or from the
// host's CSR list, for rebomos (mdp_rebomos_repack) and aeam (mdp_tile_lists_build) alike.
#include "mdp_common.h"

namespace {

// ---- tile lists -------------------------------------------------------------------------------
// Pass 1, one workgroup per tile: sweep the stencil of the tile's bounding cells; every candidate is
// tested against all atoms of the tile (broadcast LDS reads) giving a 16-bit mask of the clusters that
// list it.  Each wave takes every fourth (y,z) row and compacts its members with ballots into its own
// LDS segment (Mo from the front, S from the back); the segments are then concatenated Mo-first, so the
// result is deterministic.  Outputs: the union (tu), the masks, and the row lengths of the 16 clusters.
template <int CL>
__global__ __launch_bounds__(256) void tile_scan_kernel(const MdpGrid g, const RebomosDev P, const int nclus,
                                                        const int nlocal, const double4 *__restrict__ xq,
                                                        const int *__restrict__ perm,
                                                        const int *__restrict__ cell_start, const int cap,
                                                        int *__restrict__ tu, unsigned short *__restrict__ tmask,
                                                        int *__restrict__ tile_nu, int *__restrict__ cnt,
                                                        int *__restrict__ split, int *__restrict__ tile_flag,
                                                        const double4 *__restrict__ xq_cell)
{
  constexpr int NA = MDP_TILE * CL;
  extern __shared__ int s_dyn[];
  const int wcap = cap / 2; // per-wave segment (a wave sees about a quarter of the union)
  int *s_idx = s_dyn;                                                    // [4][wcap]
  unsigned short *s_m = (unsigned short *) (s_dyn + 4 * wcap);           // [4][wcap]
  unsigned short *s_fm = s_m + 4 * wcap;                                 // [cap] masks in final order
  __shared__ double4 s_xa[NA];
  __shared__ double s_cut[NA][2];
  __shared__ int s_lo[3], s_hi[3], s_n0[4], s_n1[4], s_over, s_rowsum;
  __shared__ double s_bb[6], s_cmax; // bounding box of the tile's atoms (lo x y z | hi x y z), their largest list cutoff
  const int t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < 3) {
    s_lo[tid] = 1 << 30;
    s_hi[tid] = -1;
  }
  if (tid == 0) s_over = s_rowsum = 0;
  __syncthreads();
  if (tid < NA) {
    const int ia = t * NA + tid;
    bool valid = ia < nlocal;
    const double4 xa = xq[valid ? ia : (nlocal > 0 ? nlocal - 1 : 0)];
    int ta = (int) xa.w;
    if (ta < 0) valid = false; // NULL-mapped atom: lists nothing
    ta = ta > 1 ? 1 : ta;      // two classes: type 0 | every other type (a style with more types sorts them out itself)
    s_xa[tid] = xa;
    s_cut[tid][0] = valid ? P.ljlist_cutsq[ta * 2 + 0] : -1.0;
    s_cut[tid][1] = valid ? P.ljlist_cutsq[ta * 2 + 1] : -1.0;
    {
      // (the NA <= 64 atom threads are the first lanes of wave 0: min / max by shuffles; absent atoms do not count)
      static_assert(NA <= 64, "the tile's atoms are held by one wave");
      double lo3[3] = {valid ? xa.x : 1.0e300, valid ? xa.y : 1.0e300, valid ? xa.z : 1.0e300};
      double hi3[3] = {valid ? xa.x : -1.0e300, valid ? xa.y : -1.0e300, valid ? xa.z : -1.0e300};
      double cm = valid ? fmax(s_cut[tid][0], s_cut[tid][1]) : -1.0;
#pragma unroll
      for (int o = 1; o < NA; o <<= 1) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
          lo3[d] = fmin(lo3[d], __shfl_xor(lo3[d], o, 64));
          hi3[d] = fmax(hi3[d], __shfl_xor(hi3[d], o, 64));
        }
        cm = fmax(cm, __shfl_xor(cm, o, 64));
      }
      if (tid == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
          s_bb[d] = lo3[d];
          s_bb[3 + d] = hi3[d];
        }
        s_cmax = cm;
      }
    }
    if (valid) {
      int cc[3];
      cc[0] = (int) ((xa.x - g.lo[0]) * g.inv[0]);
      cc[1] = (int) ((xa.y - g.lo[1]) * g.inv[1]);
      cc[2] = (int) ((xa.z - g.lo[2]) * g.inv[2]);
#pragma unroll
      for (int d = 0; d < 3; d++) {
        cc[d] = cc[d] < 0 ? 0 : (cc[d] >= g.n[d] ? g.n[d] - 1 : cc[d]);
        atomicMin(&s_lo[d], cc[d]);
        atomicMax(&s_hi[d], cc[d]);
      }
    }
  }
  __syncthreads();
  const int R = g.range;
  const bool any = s_hi[0] >= 0;
  const int xlo = max(s_lo[0] - R, 0), xhi = min(s_hi[0] + R, g.n[0] - 1);
  const int ylo = max(s_lo[1] - R, 0), yhi = min(s_hi[1] + R, g.n[1] - 1);
  const int zlo = max(s_lo[2] - R, 0), zhi = min(s_hi[2] + R, g.n[2] - 1);
  const int ny = yhi - ylo + 1, nz = zhi - zlo + 1;
  const int nrows = any ? ny * nz : 0;
  int *seg_i = s_idx + wave * wcap;
  unsigned short *seg_m = s_m + wave * wcap;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n0 = 0, n1 = 0;
  bool over = false;
  // The candidates of the (y,z) rows of cells are taken as ONE concatenated list, 64 per wave and trip: a row by
  // itself holds 15-40 atoms, so a wave walking row after row had a quarter to a half of its lanes busy in front of
  // two dependent round trips per row.  (The order in which members are found does not matter: tile_sort_fill_kernel
  // sorts every segment by atom index.)
  constexpr int kRows = 256;
  __shared__ int s_pb[kRows], s_off[kRows + 1], s_wsum[4];
  for (int rbase = 0; rbase < nrows; rbase += kRows) {
    const int nr = nrows - rbase < kRows ? nrows - rbase : kRows;
    int pb = 0, len = 0;
    if (tid < nr) {
      const int r = rbase + tid;
      const int y = ylo + r % ny, z = zlo + r / ny;
      // The stencil is a box of cells, what can hold a neighbour is the tile's bounding box grown by the largest list
      // cutoff -- about half of that box: a row of cells farther than the cutoff from the bounding box (in the y-z plane)
      // is left out, and of the others only the cells along x that the remaining distance reaches.  Conservative by
      // construction (cell and box faces, a 1e-9 A margin), so the union is what the full sweep finds.
      const double cy0 = g.lo[1] + y / g.inv[1], cy1 = g.lo[1] + (y + 1) / g.inv[1];
      const double cz0 = g.lo[2] + z / g.inv[2], cz1 = g.lo[2] + (z + 1) / g.inv[2];
      // (the first and the last cell of a dimension also hold what lies beyond the grid: that face is at infinity)
      const double dy = y < g.n[1] - 1 && s_bb[1] > cy1 ? s_bb[1] - cy1 : (y > 0 && cy0 > s_bb[4] ? cy0 - s_bb[4] : 0.0);
      const double dz = z < g.n[2] - 1 && s_bb[2] > cz1 ? s_bb[2] - cz1 : (z > 0 && cz0 > s_bb[5] ? cz0 - s_bb[5] : 0.0);
      const double left = s_cmax - dy * dy - dz * dz; // squared reach along x
      if (left >= -1.0e-9) {
        const double rx = sqrt(left > 0.0 ? left : 0.0) + 1.0e-9;
        int x0 = (int) floor((s_bb[0] - rx - g.lo[0]) * g.inv[0]), x1 = (int) floor((s_bb[3] + rx - g.lo[0]) * g.inv[0]);
        x0 = x0 < xlo ? xlo : x0;
        x1 = x1 > xhi ? xhi : x1;
        if (x0 <= x1) {
          pb = cell_start[x0 + g.n[0] * (y + g.n[1] * z)];
          len = cell_start[x1 + g.n[0] * (y + g.n[1] * z) + 1] - pb;
        }
      }
    }
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; w++) wbase += s_wsum[w];
    const int total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    s_pb[tid] = pb;
    s_off[tid] = wbase + incl - len;
    if (tid == 0) s_off[kRows] = total;
    __syncthreads();
    // the candidate of the NEXT trip is located and its two loads (position in cell order, atom index) are in flight
    // while the current one is tested against the tile's atoms: a trip was two dependent round trips to memory in
    // front of 32 distance tests, at five waves per SIMD
    const auto locate = [&](const int gi) {
      int lo = 0, hi = kRows; // s_off[lo] <= gi < s_off[hi]  (rows past nr are empty: offset = total)
#pragma unroll
      for (int it = 0; it < 8; it++) {
        const int mid = (lo + hi) >> 1;
        if (s_off[mid] <= gi) lo = mid;
        else hi = mid;
      }
      return s_pb[lo] + gi - s_off[lo];
    };
    double4 xn = make_double4(0.0, 0.0, 0.0, -1.0);
    int jn = 0;
    if (wave * 64 + lane < total) {
      const int p = locate(wave * 64 + lane);
      xn = xq_cell[p];
      jn = perm[p];
    }
    for (int g0 = wave * 64; g0 < total && !over; g0 += 256) {
      const int gi = g0 + lane;
      unsigned m = 0;
      int j = 0, tj = 0;
      const double4 xj = xn;
      const int jcur = jn;
      if (gi + 256 < total) {
        const int p = locate(gi + 256);
        xn = xq_cell[p];
        jn = perm[p];
      }
      if (gi < total) {
        j = jcur;
        tj = (int) xj.w;
        tj = tj > 1 ? 1 : tj;
        if (tj >= 0) {
#pragma unroll 8
          for (int a = 0; a < NA; a++) {
            const double4 xa = s_xa[a];
            const double dx = xa.x - xj.x, dy = xa.y - xj.y, dz = xa.z - xj.z;
            if (dx * dx + dy * dy + dz * dz <= s_cut[a][tj]) m |= 1u << (a / CL);
          }
        }
      }
      const bool k0 = m != 0 && tj == 0, k1 = m != 0 && tj != 0;
      const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1);
      const int c0 = __popcll(b0), c1 = __popcll(b1);
      if (n0 + n1 + c0 + c1 > wcap) {
        over = true;
        break;
      }
      if (k0) {
        const int pos = n0 + __popcll(b0 & below);
        seg_i[pos] = j;
        seg_m[pos] = (unsigned short) m;
      }
      if (k1) {
        const int pos = wcap - 1 - (n1 + __popcll(b1 & below));
        seg_i[pos] = j;
        seg_m[pos] = (unsigned short) m;
      }
      n0 += c0;
      n1 += c1;
    }
    __syncthreads(); // (s_pb / s_off are rewritten by the next block of rows)
  }
  if (lane == 0) {
    s_n0[wave] = n0;
    s_n1[wave] = n1;
    if (over) s_over = 1;
  }
  __syncthreads();
  const int N0 = s_n0[0] + s_n0[1] + s_n0[2] + s_n0[3];
  const int N1 = s_n1[0] + s_n1[1] + s_n1[2] + s_n1[3];
  int nU = N0 + N1;
  if (s_over || nU > cap - 1) { // (slot nU is the kernel's dummy entry, so nU <= cap-1)
    if (tid == 0) {
      atomicOr(&tile_flag[0], 1);
      tile_nu[2 * t] = tile_nu[2 * t + 1] = 0;
    }
    if (tid < MDP_TILE) cnt[t * MDP_TILE + tid] = split[t * MDP_TILE + tid] = 0;
    return;
  }
  int base0 = 0, base1 = N0;
  for (int w = 0; w < wave; w++) {
    base0 += s_n0[w];
    base1 += s_n1[w];
  }
  int *mem = tu + (size_t) t * cap;
  unsigned short *mm = tmask + (size_t) t * cap;
  for (int i = lane; i < n0; i += 64) {
    const int u = base0 + i;
    const unsigned short m = seg_m[i];
    mem[u] = seg_i[i];
    mm[u] = m;
    s_fm[u] = m;
  }
  for (int i = lane; i < n1; i += 64) {
    const int u = base1 + i, src = wcap - 1 - i;
    const unsigned short m = seg_m[src];
    mem[u] = seg_i[src];
    mm[u] = m;
    s_fm[u] = m;
  }
  __syncthreads();
  const int gq = tid / 16, sq = tid % 16;
  int c0 = 0, c1 = 0;
  for (int u = sq; u < nU; u += 16) {
    const int bit = (s_fm[u] >> gq) & 1;
    c0 += u < N0 ? bit : 0;
    c1 += u < N0 ? 0 : bit;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64);
    c1 += __shfl_xor(c1, o, 64);
  }
  // Row layout: every tile has MDP_TILE rows (absent clusters get all-dummy rows); both segments are padded
  // with the dummy index to whole 16-lane steps AND to the longest of the four clusters that share a wave
  // in the compute kernel, so that its loops are wave-uniform (idle lanes would cost the same time).
  int p0 = (c0 + 15) & ~15, p1 = (c1 + 15) & ~15;
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    p0 = max(p0, __shfl_xor(p0, o, 64));
    p1 = max(p1, __shfl_xor(p1, o, 64));
  }
  const int kc = t * MDP_TILE + gq;
  if (sq == 0) {
    cnt[kc] = p0 + p1;
    split[kc] = p0;
    atomicAdd(&s_rowsum, p0 + p1);
  }
  __syncthreads();
  if (tid == 0) {
    tile_nu[2 * t] = nU;
    tile_nu[2 * t + 1] = N0;
    // running maxima over all tiles, two words for the whole grid.  A look first -- the word only grows, so a stale smaller
    // value costs at most a redundant atomic -- leaves a handful of atomics per launch instead of two per tile on ONE
    // address (the look goes to the L2, where the atomics land: a CU's L1 would keep the first value it saw).  Measured:
    // no difference at 124 416 tiles (the atomics are fire-and-forget at the end of a workgroup); the per-WAVE atomics
    // with a return value in classify_kernel were the ones that cost a millisecond.
    if (nU > __hip_atomic_load(&tile_flag[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&tile_flag[1], nU);
    if (s_rowsum > __hip_atomic_load(&tile_flag[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(&tile_flag[2], s_rowsum); // row entries of the whole tile (kernels that stage a tile's rows in LDS)
  }
}

// tile_scan_kernel with the union gathered from the host rows of the tile's atoms: the same atom is listed by many of
// them, so the members go through a hash table in LDS (key = atom index, value = the 16-bit cluster mask | element
// class << 16) and are compacted element 0 first.  tile_sort_fill_kernel orders every segment by atom index afterwards, so
// the order of insertion leaves no trace.
template <int CL>
__global__ __launch_bounds__(256) void tile_scan_csr_kernel(const RebomosDev P, const int nclus, const int nlocal,
                                                            const double4 *__restrict__ xq,
                                                            const long long *__restrict__ nb_off,
                                                            const int *__restrict__ nb, const int cap,
                                                            int *__restrict__ tu, unsigned short *__restrict__ tmask,
                                                            int *__restrict__ tile_nu, int *__restrict__ cnt,
                                                            int *__restrict__ split, int *__restrict__ tile_flag)
{
  constexpr int NA = MDP_TILE * CL;
  extern __shared__ int s_dyn[];
  const int HS = 2 * cap; // (power of two: cap is)
  int *s_key = s_dyn;                                       // [HS]
  int *s_val = s_dyn + HS;                                  // [HS]
  unsigned short *s_fm = (unsigned short *) (s_dyn + 2 * HS); // [cap] masks in final order
  __shared__ double4 s_xa[NA];
  __shared__ double s_cut[NA][2];
  __shared__ int s_count, s_over, s_rowsum, s_w0[4], s_w1[4];
  const int t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int h = tid; h < HS; h += 256) {
    s_key[h] = -1;
    s_val[h] = 0;
  }
  if (tid == 0) s_count = s_over = s_rowsum = 0;
  if (tid < NA) {
    const int ia = t * NA + tid;
    bool valid = ia < nlocal;
    const double4 xa = xq[valid ? ia : (nlocal > 0 ? nlocal - 1 : 0)];
    int ta = (int) xa.w;
    if (ta < 0) valid = false;
    ta = ta > 1 ? 1 : ta;
    s_xa[tid] = xa;
    s_cut[tid][0] = valid ? P.ljlist_cutsq[ta * 2 + 0] : -1.0;
    s_cut[tid][1] = valid ? P.ljlist_cutsq[ta * 2 + 1] : -1.0;
  }
  __syncthreads();
  // every wave walks the rows of NA/4 atoms, 64 entries a trip
  for (int a = wave; a < NA; a += 4) {
    const int ia = t * NA + a;
    if (ia >= nlocal || s_cut[a][0] < 0.0) continue; // (wave-uniform)
    const double4 xa = s_xa[a];
    const long long b = nb_off[ia];
    const int len = (int) (nb_off[ia + 1] - b);
    for (int k = lane; k < len; k += 64) {
      const int j = nb[b + k];
      const double4 xj = xq[j];
      int tj = (int) xj.w;
      tj = tj > 1 ? 1 : tj;
      if (tj < 0 || j == ia) continue; // (the host lists no atom in its own row; guarded anyway)
      const double dx = xa.x - xj.x, dy = xa.y - xj.y, dz = xa.z - xj.z;
      if (!(dx * dx + dy * dy + dz * dz <= s_cut[a][tj])) continue;
      const int val = (1 << (a / CL)) | (tj << 16);
      unsigned h = ((unsigned) j * 2654435761u) & (unsigned) (HS - 1);
      for (int probe = 0; probe < HS; probe++) {
        const int old = atomicCAS(&s_key[h], -1, j);
        if (old == -1) {
          if (atomicAdd(&s_count, 1) >= cap - 1) s_over = 1; // (slot nU is the kernels' dummy entry: nU <= cap - 1)
        }
        if (old == -1 || old == j) {
          atomicOr(&s_val[h], val);
          break;
        }
        h = (h + 1) & (unsigned) (HS - 1);
      }
    }
  }
  __syncthreads();
  if (s_over) {
    if (tid == 0) {
      atomicOr(&tile_flag[0], 1);
      tile_nu[2 * t] = tile_nu[2 * t + 1] = 0;
    }
    if (tid < MDP_TILE) cnt[t * MDP_TILE + tid] = split[t * MDP_TILE + tid] = 0;
    return;
  }
  // compaction: thread tid owns the slots [tid * HS/256, (tid+1) * HS/256)
  const int per = HS / 256;
  int m0 = 0, m1 = 0;
  for (int q = 0; q < per; q++) {
    const int h = tid * per + q;
    if (s_key[h] >= 0) {
      if ((s_val[h] >> 16) & 1) m1++;
      else m0++;
    }
  }
  int i0 = m0, i1 = m1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u0 = __shfl_up(i0, o, 64), u1 = __shfl_up(i1, o, 64);
    if (lane >= o) {
      i0 += u0;
      i1 += u1;
    }
  }
  if (lane == 63) {
    s_w0[wave] = i0;
    s_w1[wave] = i1;
  }
  __syncthreads();
  const int N0 = s_w0[0] + s_w0[1] + s_w0[2] + s_w0[3];
  const int N1 = s_w1[0] + s_w1[1] + s_w1[2] + s_w1[3];
  const int nU = N0 + N1;
  int p0 = i0 - m0, p1 = N0 + i1 - m1;
  for (int w = 0; w < wave; w++) {
    p0 += s_w0[w];
    p1 += s_w1[w];
  }
  int *mem = tu + (size_t) t * cap;
  unsigned short *mm = tmask + (size_t) t * cap;
  for (int q = 0; q < per; q++) {
    const int h = tid * per + q;
    const int j = s_key[h];
    if (j < 0) continue;
    const int v = s_val[h];
    const int u = ((v >> 16) & 1) ? p1++ : p0++;
    mem[u] = j;
    mm[u] = (unsigned short) (v & 0xFFFF);
    s_fm[u] = (unsigned short) (v & 0xFFFF);
  }
  __syncthreads();
  // row lengths: as tile_scan_kernel
  const int gq = tid / 16, sq = tid % 16;
  int c0 = 0, c1 = 0;
  for (int u = sq; u < nU; u += 16) {
    const int bit = (s_fm[u] >> gq) & 1;
    c0 += u < N0 ? bit : 0;
    c1 += u < N0 ? 0 : bit;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64);
    c1 += __shfl_xor(c1, o, 64);
  }
  int q0 = (c0 + 15) & ~15, q1 = (c1 + 15) & ~15;
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    q0 = max(q0, __shfl_xor(q0, o, 64));
    q1 = max(q1, __shfl_xor(q1, o, 64));
  }
  const int kc = t * MDP_TILE + gq;
  if (sq == 0) {
    cnt[kc] = q0 + q1;
    split[kc] = q0;
    atomicAdd(&s_rowsum, q0 + q1);
  }
  __syncthreads();
  if (tid == 0) {
    tile_nu[2 * t] = nU;
    tile_nu[2 * t + 1] = N0;
    if (nU > __hip_atomic_load(&tile_flag[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&tile_flag[1], nU);
    if (s_rowsum > __hip_atomic_load(&tile_flag[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&tile_flag[2], s_rowsum);
  }
}

// Between the passes: the members of a union are sorted by atom index (each element segment by itself).  The
// kernels that stage a union gather xq[member] with consecutive lanes taking consecutive members; atoms are stored
// along a Hilbert curve, so after the sort neighbouring lanes mostly hit the same 128-byte line (four atoms) instead
// of one line each -- the staging gathers were a quarter of the L1 lookups of the AEAM tile kernels.
// The sort and pass 2 (tile_fill_kernel below, which serves alone with MDP_TILE_SORT=0) in one launch: the sorted masks
// stay in LDS and the rows are filled from there -- the masks of a tile are needed by nothing else, so their way back to
// global memory and a launch with its dependent loads (tile -> union size -> masks) are saved.
__global__ __launch_bounds__(256) void tile_sort_fill_kernel(const int cap, const int np_max, const int *__restrict__ tile_nu,
                                                             int *__restrict__ tu, const unsigned short *__restrict__ tmask,
                                                             const int nclus, const long long *__restrict__ off,
                                                             const int *__restrict__ split, unsigned short *__restrict__ lj16)
{
  extern __shared__ unsigned long long s_key[];                                   // [np_max] keys of the segment being sorted
  unsigned short *s_fm = reinterpret_cast<unsigned short *>(s_key + np_max);      // [cap] masks in final order
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int nU = tile_nu[2 * t], N0 = tile_nu[2 * t + 1];
  int *mem = tu + (size_t) t * cap;
  const unsigned short *mm = tmask + (size_t) t * cap;
  // (everything the fill needs from global memory is requested before the sort)
  const int gq = tid / 16, sq = tid % 16, glane0 = lane - sq;
  const int kc = t * MDP_TILE + gq;
  const bool have = kc < nclus;
  const long long b0 = off[kc];
  const int len[2] = {split[kc], (int) (off[kc + 1] - b0) - split[kc]}; // padded segment lengths (tile_scan_kernel)
  for (int seg = 0; seg < 2; seg++) {
    const int b = seg ? N0 : 0, n = (seg ? nU : N0) - b;
    if (n <= 1) { // (block-uniform)
      if (n == 1 && tid == 0) s_fm[b] = mm[b];
      continue;
    }
    int np = 2;
    while (np < n) np <<= 1;
    for (int i = tid; i < np; i += 256)
      s_key[i] = i < n ? (((unsigned long long) (unsigned) mem[b + i]) << 16) | mm[b + i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int q = tid; q < (np >> 1); q += 256) {
          const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), p = i | j;
          const unsigned long long x = s_key[i], y = s_key[p];
          if ((x > y) == ((i & k) == 0)) {
            s_key[i] = y;
            s_key[p] = x;
          }
        }
        __syncthreads();
      }
    for (int i = tid; i < n; i += 256) {
      const unsigned long long v = s_key[i];
      mem[b + i] = (int) (v >> 16);
      s_fm[b + i] = (unsigned short) (v & 0xFFFFull);
    }
    __syncthreads();
  }
  __syncthreads();
  unsigned short *row = lj16 + b0;
  const unsigned long long below = (1ull << sq) - 1ull;
  for (int seg = 0; seg < 2; seg++) {
    const int ub = seg ? N0 : 0, ue = seg ? nU : N0;
    int n = 0;
    for (int base = ub; base < ue; base += 16) {
      const int u = base + sq;
      const bool k = have && u < ue && ((s_fm[u < ue ? u : ub] >> gq) & 1);
      const unsigned long long bal = (__ballot(k) >> glane0) & 0xFFFFull;
      if (k) row[n + __popcll(bal & below)] = (unsigned short) u;
      n += __popcll(bal);
    }
    for (int q = n + sq; q < len[seg]; q += 16) row[q] = (unsigned short) nU; // padding: the dummy slot
    row += len[seg];
  }
}

// Pass 2: each cluster (16 lanes) walks its tile's masks in union order and keeps the entries with its bit;
// the Mo segment and the S segment are each padded to a whole 16-lane step with the dummy index nU
__global__ __launch_bounds__(256) void tile_fill_kernel(const int nclus, const int cap,
                                                        const int *__restrict__ tile_nu,
                                                        const unsigned short *__restrict__ tmask,
                                                        const long long *__restrict__ off,
                                                        const int *__restrict__ split,
                                                        unsigned short *__restrict__ lj16)
{
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int gq = tid / 16, sq = tid % 16, glane0 = lane - sq;
  const int kc = t * MDP_TILE + gq;
  const bool have = kc < nclus;
  const int nU = tile_nu[2 * t], N0 = tile_nu[2 * t + 1];
  const unsigned short *mm = tmask + (size_t) t * cap;
  const long long b = off[kc];
  const int len[2] = {split[kc], (int) (off[kc + 1] - b) - split[kc]}; // padded segment lengths (tile_scan_kernel)
  unsigned short *row = lj16 + b;
  const unsigned long long below = (1ull << sq) - 1ull;
  for (int seg = 0; seg < 2; seg++) {
    const int ub = seg ? N0 : 0, ue = seg ? nU : N0;
    int n = 0;
    for (int base = ub; base < ue; base += 16) {
      const int u = base + sq;
      const bool k = have && u < ue && ((mm[u] >> gq) & 1);
      const unsigned long long bal = (__ballot(k) >> glane0) & 0xFFFFull;
      if (k) row[n + __popcll(bal & below)] = (unsigned short) u;
      n += __popcll(bal);
    }
    for (int q = n + sq; q < len[seg]; q += 16) row[q] = (unsigned short) nU; // padding: the dummy slot
    row += len[seg];
  }
}

// Dynamic pruning of the rows (between list builds): every row entry is tested against the cluster's atoms at
// the CURRENT positions and kept when it lies within (upper window bound + buffer) of one of them; the kept entries
// are compacted into a second set of rows at the same offsets (segments padded as tile_scan_kernel pads them).
// The list skin -- a third of the entries of a list built with 1 A of it -- then costs a pass of this kernel every
// few tens of steps instead of an evaluation in every step; the rows as built stay, the buffer has its own
// displacement trigger (moved_kernel), and an entry is never missed: it enters a window only after the two atoms
// together moved the buffer, i.e. one of them half of it.
struct PruneLimits {
  double rsq[4]; // (window upper bound + buffer)^2 per pair type ti * 2 + tj
};
template <int CL>
__global__ __launch_bounds__(256) void tile_prune_kernel(const PruneLimits lim, const int nlocal, const int nclus,
                                                         const double4 *__restrict__ xq, const int cap, const int capL,
                                                         const int *__restrict__ tu, const int *__restrict__ tile_nu,
                                                         const long long *__restrict__ lj_off,
                                                         const int *__restrict__ lj_split,
                                                         const unsigned short *__restrict__ lj16,
                                                         unsigned short *__restrict__ lj16_in,
                                                         int *__restrict__ len_in, int *__restrict__ split_in)
{
  // The tile's rows (contiguous in memory) are staged in LDS with 16-byte loads, compacted there in place -- a
  // row's kept entries never outrun its read position, and a row belongs to one 16-lane group of one wave -- and
  // written back whole with 16-byte stores: no 2-byte global traffic, no global load inside the loop.  What lies
  // behind a row's new length stays what it was (valid indices: the kernels read a few entries past a segment).
  constexpr int L = 16, SK = 3;
  extern __shared__ double s_pos[]; // [capL][3], then the rows
  unsigned short *__restrict__ s_rows = reinterpret_cast<unsigned short *>(s_pos + 3 * (size_t) capL);
  const int tid = threadIdx.x, lane = tid & 63, s = lane % L, glane0 = lane - s;
  const int t = blockIdx.x;
  const int kc = t * MDP_TILE + tid / L;
  const int nU = tile_nu[2 * t];
  const int *__restrict__ mem = tu + (size_t) t * cap;
  const long long rb = lj_off[(size_t) t * MDP_TILE];
  const int rtot = (int) (lj_off[(size_t) t * MDP_TILE + MDP_TILE] - rb); // entries of the whole tile (multiple of 16)
  {
    int sidx[SK];
#pragma unroll
    for (int k = 0; k < SK; k++) sidx[k] = mem[tid + 256 * k]; // (rows are cap >= 2048 long: always in bounds)
    double4 sv[SK];
#pragma unroll
    for (int k = 0; k < SK; k++) sv[k] = xq[tid + 256 * k < nU ? sidx[k] : 0];
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(lj16 + rb);
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(s_rows);
    for (int e = tid; e * 8 < rtot; e += 256) dst[e] = src[e];
#pragma unroll
    for (int k = 0; k < SK; k++) {
      const int u = tid + 256 * k;
      if (u < nU) {
        s_pos[3 * u] = sv[k].x;
        s_pos[3 * u + 1] = sv[k].y;
        s_pos[3 * u + 2] = sv[k].z;
      }
    }
    for (int u = tid + 256 * SK; u < nU; u += 256) {
      const double4 v = xq[mem[u]];
      s_pos[3 * u] = v.x;
      s_pos[3 * u + 1] = v.y;
      s_pos[3 * u + 2] = v.z;
    }
  }
  const long long b = lj_off[kc];
  const int cnt = __builtin_amdgcn_readfirstlane((int) (lj_off[kc + 1] - b));
  const int split = __builtin_amdgcn_readfirstlane(lj_split[kc]);
  unsigned short *__restrict__ row = s_rows + (int) (b - rb);
  double4 xa[CL];
  bool real[CL];
  int ta[CL];
#pragma unroll
  for (int c = 0; c < CL; c++) {
    const int ia = kc * CL + c;
    real[c] = kc < nclus && ia < nlocal;
    xa[c] = xq[real[c] ? ia : nlocal - 1];
    ta[c] = (int) xa[c].w;
    if (ta[c] < 0) { // type mapped to NULL: takes part in nothing
      real[c] = false;
      ta[c] = 0;
    }
    ta[c] = ta[c] > 1 ? 1 : ta[c]; // (the two classes of tile_scan_kernel)
  }
  __syncthreads();
  const unsigned long long below = (1ull << s) - 1ull;
  int pseg[2];
  int base = 0;
#pragma unroll
  for (int seg = 0; seg < 2; seg++) {
    const int kb = seg ? split : 0, ke = seg ? cnt : split;
    double lim_c[CL];
#pragma unroll
    for (int c = 0; c < CL; c++) lim_c[c] = lim.rsq[ta[c] * 2 + seg];
    int n = 0;
    for (int k = kb; k < ke; k += L) { // (segments are whole 16-lane steps, equally long for the rows of a wave)
      const int li = (int) row[k + s];
      bool keep = false;
      if (li < nU) {
        const double xj = s_pos[3 * li], yj = s_pos[3 * li + 1], zj = s_pos[3 * li + 2];
#pragma unroll
        for (int c = 0; c < CL; c++) {
          const double dx = xa[c].x - xj, dy = xa[c].y - yj, dz = xa[c].z - zj;
          keep = keep || (real[c] && dx * dx + dy * dy + dz * dz <= lim_c[c]);
        }
      }
      const unsigned long long gb = (__ballot(keep) >> glane0) & 0xFFFFull;
      // (the read of this trip is complete for the whole wave before any lane writes: same instruction stream)
      if (keep) row[base + n + __popcll(gb & below)] = (unsigned short) li;
      n += __popcll(gb);
    }
    int p = (n + 15) & ~15;
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) p = max(p, __shfl_xor(p, o, 64));
    for (int q = n + s; q < p; q += L) row[base + q] = (unsigned short) nU; // padding: the dummy slot
    pseg[seg] = p;
    base += p;
  }
  if (s == 0) {
    split_in[kc] = pseg[0];
    len_in[kc] = pseg[0] + pseg[1];
  }
  __syncthreads();
  {
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(s_rows);
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(lj16_in + rb);
    for (int e = tid; e * 8 < rtot; e += 256) dst[e] = src[e];
  }
}

} // namespace

// Sorts the unions and writes the rows in one launch; *filled stays false with MDP_TILE_SORT=0 (the unions stay as found
// and tile_fill_kernel writes the rows).
static int tile_sort_launch(mdp_ctx *c, const int ntile, const int nclus, bool *filled)
{
  *filled = false;
  if (const char *e = getenv("MDP_TILE_SORT"))
    if (atoi(e) == 0) return MDP_OK;
  int np = 2;
  while (np < c->tile_maxu) np <<= 1;
  const size_t lds = (size_t) np * sizeof(unsigned long long) + (size_t) c->tile_cap * sizeof(unsigned short);
  MDP_TRY(mdp_launch(c, tile_sort_fill_kernel, ntile, 256, lds, c->stream, c->tile_cap, np, c->tile_nu.p, c->tu.p, c->tmask.p,
                     nclus, c->lj_off.p, c->lj_split.p, c->lj16.p));
  *filled = true;
  return MDP_OK;
}

// pass 1 over all tiles at union capacity `cap`, members from the bin grid or from the host's CSR list
template <int CL> static int tile_scan_launch(mdp_ctx *c, const RebomosDev &P, const bool from_csr, const int ntile, const int nclus, const int cap)
{
  if (from_csr) // hash table of 2 cap (key, value) slots + cap masks
    return mdp_launch(c, tile_scan_csr_kernel<CL>, ntile, 256, (size_t) 18 * cap, c->stream, P, nclus, c->nlocal, c->xq.p,
                      c->nb_off.p, c->nb.p, cap, c->tu.p, c->tmask.p, c->tile_nu.p, c->lj_cnt.p, c->lj_split.p, c->tile_flag.p);
  // 4 wave segments of cap/2 (int + ushort) + cap ushort
  return mdp_launch(c, tile_scan_kernel<CL>, ntile, 256, (size_t) 14 * cap, c->stream, c->grid, P, nclus, c->nlocal, c->xq.p,
                    c->cell_perm.p, c->cell_start.p, cap, c->tu.p, c->tmask.p, c->tile_nu.p, c->lj_cnt.p, c->lj_split.p,
                    c->tile_flag.p, c->xq_cell.p);
}

// The one builder of the tile rows (mdp_common.h).  Fills tu / tile_nu / lj_off / lj_split / lj16 and c->nclus, ntile,
// tile_cap, tile_maxu, tile_rowmax, lj_total, tile_rows_cl; leaves the context as it was and *ok = false when a union
// outgrows what LDS can stage (cap 4096).
int mdp_tile_rows_build(mdp_ctx *c, const RebomosDev &P, int cl, const bool from_csr, const MdpRead *ride, bool *ok)
{
  *ok = false;
  hipStream_t st = c->stream;
  if (cl != 1) cl = 2;
  const int nclus = (c->nlocal + cl - 1) / cl;
  if (nclus <= 0) return MDP_OK;
  const int ntile = (nclus + MDP_TILE - 1) / MDP_TILE;
  const int nrow = ntile * MDP_TILE; // every tile has MDP_TILE rows
  MDP_HIP(c, c->lj_split.reserve(nrow + 1));
  MDP_HIP(c, c->lj_cnt.reserve(nrow + 1));
  MDP_HIP(c, c->lj_off.reserve(nrow + 2));
  MDP_HIP(c, c->tile_flag.reserve(4));
  MDP_HIP(c, c->tile_nu.reserve((size_t) 2 * ntile + 2));
  MDP_HIP(c, c->lj_fix_stamp.reserve((size_t) ntile + 1));
  MDP_HIP(c, hipMemsetAsync(c->lj_fix_stamp.p, 0, sizeof(int) * ((size_t) ntile + 1), st)); // (no compute has stamp 0; aeam never reads it)
  for (int cap = c->tile_cap > 0 ? c->tile_cap : 2048;; cap *= 2) { // (a union outgrew the segment: retry larger ...
    if (cap > 4096) return MDP_OK;                                    //  ... and give up beyond what LDS can stage)
    MDP_HIP(c, c->tu.reserve((size_t) ntile * cap));
    MDP_HIP(c, c->tmask.reserve((size_t) ntile * cap));
    MDP_HIP(c, hipMemsetAsync(c->tile_flag.p, 0, sizeof(int) * 3, st));
    MDP_TRY(cl == 1 ? tile_scan_launch<1>(c, P, from_csr, ntile, nclus, cap) : tile_scan_launch<2>(c, P, from_csr, ntile, nclus, cap));
    int tf[3] = {0, 0, 0};
    MDP_TRY(mdp_read_one(c, c->tile_flag.p, sizeof(int) * 3, tf));
    if (!tf[0]) {
      c->tile_cap = cap;
      c->tile_maxu = tf[1];
      c->tile_rowmax = tf[2];
      break;
    }
  }
  MDP_TRY(mdp_scan_exclusive_i64(c, c->lj_cnt.p, c->lj_off.p, nrow));
  long long total = 0;
  {
    const MdpRead rd[2] = {{c->lj_off.p + nrow, sizeof(long long), &total}, ride ? *ride : MdpRead{nullptr, 0, nullptr}};
    MDP_TRY(mdp_read_small(c, rd, ride ? 2 : 1));
  }
  MDP_HIP(c, c->lj16.reserve((size_t) total + 256)); // slack: rows are read a few steps past their end
  bool rows_filled = false;
  MDP_TRY(tile_sort_launch(c, ntile, nclus, &rows_filled));
  if (!rows_filled) // (MDP_TILE_SORT=0: the unions stay as found)
    MDP_TRY(mdp_launch(c, tile_fill_kernel, ntile, 256, 0, st, nclus, c->tile_cap, c->tile_nu.p, c->tmask.p, c->lj_off.p,
                       c->lj_split.p, c->lj16.p));
  c->nclus = nclus;
  c->ntile = ntile;
  c->lj_total = total;
  c->tile_rows_cl = cl;
  mdp_rows_renewed(c);
  *ok = true;
  return MDP_OK;
}

// The tile rows for another two-type style (aeam): `cutsq[ti*2+tj]` = squared list radius of the pair; needs the bin
// grid of the current positions (mdp_bin_atoms).  *ok = false when a union does not fit (caller keeps its CSR path).
int mdp_tile_lists_build(mdp_ctx *c, const double cutsq[4], int cl, bool *ok)
{
  RebomosDev P = {};
  for (int k = 0; k < 4; k++) P.ljlist_cutsq[k] = cutsq[k];
  MDP_TRY(mdp_tile_rows_build(c, P, cl, /*from_csr=*/false, nullptr, ok));
  if (*ok && getenv("MDP_DEBUG"))
    fprintf(stderr, "[mdp] tile lists (generic): %d tiles, cap %d, largest union %d, %.1f row entries per cluster\n", c->ntile,
            c->tile_cap, c->tile_maxu, (double) c->lj_total / c->nclus);
  return MDP_OK;
}

// (Re-)prune the tile rows from the current positions (tile_prune_kernel) and remember those positions.
// lim_rsq[ti * 2 + tj]: (largest pair distance the kernels act on + buffer)^2.
static int tile_prune(mdp_ctx *c, const double lim_rsq[4])
{
  hipStream_t st = c->stream;
  const int nrow = c->ntile * MDP_TILE;
  MDP_HIP(c, c->lj_len_in.reserve(nrow + 1));
  MDP_HIP(c, c->lj_split_in.reserve(nrow + 1));
  MDP_HIP(c, c->xhold_prune.reserve((size_t) 3 * c->nall + 3));
  if (c->prune_copied_epoch != c->prune_epoch) { // rows were rebuilt: the slack behind the last row as well
    MDP_HIP(c, c->lj16_in.reserve((size_t) c->lj_total + 256)); // (reads past a segment's end must find valid indices)
    MDP_HIP(c, hipMemcpyAsync(c->lj16_in.p + c->lj_total, c->lj16.p + c->lj_total, sizeof(unsigned short) * 256,
                              hipMemcpyDeviceToDevice, st));
    c->prune_copied_epoch = c->prune_epoch;
  }
  PruneLimits lim;
  for (int k = 0; k < 4; k++) lim.rsq[k] = lim_rsq[k];
  const int capL = (c->tile_maxu + 1 + 1) & ~1; // (the rows behind it start 16-byte aligned)
  const size_t lds = (size_t) capL * 3 * sizeof(double) + (size_t) 2 * c->tile_rowmax + 32;
  if (c->tile_rowmax <= 0 || lds > 160 * 1024) { // (rows of a tile do not fit LDS next to its union: no pruning)
    c->prune_valid = false;
    return MDP_OK;
  }
  const auto kernel = c->tile_rows_cl == 1 ? tile_prune_kernel<1> : tile_prune_kernel<2>;
  MDP_TRY(mdp_launch(c, kernel, c->ntile, 256, lds, st, lim, c->nlocal, c->nclus, c->xq.p, c->tile_cap, capL, c->tu.p,
                     c->tile_nu.p, c->lj_off.p, c->lj_split.p, c->lj16.p, c->lj16_in.p, c->lj_len_in.p, c->lj_split_in.p));
  MDP_TRY(mdp_hold(c, c->nall, c->xhold_prune.p));
  c->prune_valid = true;
  c->prune_stale = false;
  c->prune_epoch++; // (a displacement check launched before this says nothing about the new reference)
  c->prune_copied_epoch = c->prune_epoch;
  c->prunes++;
  c->computes_since_prune = 0;
  return MDP_OK;
}

// the buffer adapts like the inner skin: a pruning costs about a third of a pass over the rows, so a trigger that
// fires within a dozen computes (thermal vibration reaching half the buffer) widens it, one that stays quiet for
// long narrows it.  fired: the trigger of the current pruning has fired (MDP_PRUNE_BUFFER fixes the buffer).
static void prune_adapt(mdp_ctx *c, const double buf_max, const bool fired)
{
  const char *eb = getenv("MDP_PRUNE_BUFFER");
  const double fixed_buf = eb ? atof(eb) : 0.0;
  if (fixed_buf > 0.0) {
    c->prune_buf = fixed_buf;
    return;
  }
  if (!fired) return;
  if (c->computes_since_prune < 12 && c->prune_buf + 0.1 <= buf_max + 1e-9) c->prune_buf += 0.1;
  else if (c->computes_since_prune > 60 && c->prune_buf - 0.05 >= 0.2 - 1e-9) c->prune_buf -= 0.05;
}

// Keeps the pruned rows current: adapts the buffer and prunes (again) when the rows are new or the buffer's trigger has
// fired.  Call before the first kernel that walks the rows; positions (ghosts included) must be current -- unless
// may_prune is false: then a pruning that is due is only reported (*due; the caller comes back once the halo has
// arrived).  cut[ti * 2 + tj]: the largest pair distance the kernels act on; skin: the skin of the rows as built.
// own_check: the style runs the displacement checks itself and has read their flags (rebomos_lists_stale), in host mode
// as well, and prunes one-atom rows too.  A style without (aeam) prunes in resident runs only, on the flags the integrate
// kernel and the halo unpack of the previous step left (MdpStyleCheck), which are collected here, and only two-atom rows.
int mdp_prune_upkeep(mdp_ctx *c, const double cut[4], const double skin, const bool own_check, const bool may_prune, bool *due)
{
  if (due) *due = false;
  const char *ep = getenv("MDP_PRUNE");
  const int prune_on = ep ? atoi(ep) : 1;
  if (!prune_on || c->ntile <= 0 || (!own_check && (!c->md || c->tile_rows_cl != 2))) {
    c->prune_valid = false;
    return MDP_OK;
  }
  if (!own_check) MDP_TRY(mdp_sflag_collect(c, nullptr, nullptr));
  prune_adapt(c, skin - 0.2, c->prune_valid && c->prune_stale);
  if (!(c->prune_buf < skin)) { // (a buffer as wide as the skin prunes nothing)
    c->prune_valid = false;
    return MDP_OK;
  }
  if (!c->prune_valid || c->prune_stale) {
    if (!may_prune) {
      if (due) *due = true;
      return MDP_OK;
    }
    double lim[4];
    for (int k = 0; k < 4; k++) lim[k] = (cut[k] + c->prune_buf) * (cut[k] + c->prune_buf);
    MDP_TRY(tile_prune(c, lim));
  }
  c->computes_since_prune++;
  return MDP_OK;
}
