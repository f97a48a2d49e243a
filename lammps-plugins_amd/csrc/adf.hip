// adf.hip -- bond-angle histograms of a device-resident run (LAMMPS compute adf), in integers.
// A read bins ALL atoms of the brick (owned and ghost) as a read of rdf.hip does (mdp_measure_bin, measure_bin.hip) at cell
// width >= half the largest outer radius, into buffers that belong to MdpAdf.  Then one WAVE per centre at a time, four
// centres in flight per workgroup:
//   phase A  the 64 lanes stride over the candidates of the centre's 5 x 5 stencil runs, laid end to end (measure_walk.h), test rsq against
//            the largest outer radius, form the candidate's j- and k-masks (the triples whose type range and shell it fits, among those the
//            centre belongs to) and compact the hits by ballot and prefix count into the wave's short list in LDS
//            {dx, dy, dz, 1 / r, jmask, kmask}, MDP_ADF_MAXNEIGH entries;
//   phase B  the lanes stride over the n^2 ordered pairs (a, b) of the list; for m = jmask[a] & kmask[b] != 0 and a != b they
//            form the cosine, the ordinate and the bin, and add 1 to the 32-bit LDS counter [triple][bin] of every set bit.
// A centre with more hits than the list holds is counted, not truncated, and the read is refused.  The workgroup's non-zero
// counters go to the global 64-bit histogram with device-scope integer atomics.  No floating-point atomic anywhere: two
// reads of one state agree exactly, and the sum over the bricks of a decomposition is the one-brick histogram wherever
// the last bit of an ordinate does not decide the bin.
#include "measure_walk.h"

namespace {

constexpr int kAdfWaves = 4;           // waves of a workgroup, each with a short list of its own
constexpr int kAdfChunksPerFlush = 64; // a workgroup flushes its 32-bit counters after this many chunks of 256 places: a centre
                                       // adds at most MDP_ADF_MAXNEIGH^2 = 2^14 hits to a counter, a chunk has at most 2^8
                                       // centres, so a counter stays below 2^14 * 2^8 * 2^6 = 2^28
constexpr int kAdfCntWords = MDP_ADF_MAXTRIPLE + 2; // icount per triple, the centres over the cap, the atoms whose tag has no entry

using Grid = MdpGrid;

// squared shell radii per triple, and per type code the triples whose i, j and k range holds the type
struct AdfTab {
  double rsq[4][MDP_ADF_MAXTRIPLE]; // j inner, j outer, k inner, k outer
  unsigned imask[kBinTypes], jmask[kBinTypes], kmask[kBinTypes];
};
constexpr int kAdfTabWords = (int) (sizeof(AdfTab) / sizeof(unsigned));
// the short list of a wave: the centre's neighbours inside the largest outer radius
struct AdfList {
  double dx[MDP_ADF_MAXNEIGH], dy[MDP_ADF_MAXNEIGH], dz[MDP_ADF_MAXNEIGH], inv[MDP_ADF_MAXNEIGH];
  unsigned jm[MDP_ADF_MAXNEIGH], km[MDP_ADF_MAXNEIGH];
  MdpWalkRuns runs; // the 25 runs of the centre's stencil
};
// LDS of a workgroup, in bytes: the table, four lists ((40 B x 128 + 256 B) x 4 = 21 KB), the histogram, the counters: 55.6 KB at
// the most (8 192 counters), 23 KB with a small histogram
size_t adf_lds_bytes(const int nhist) { return sizeof(AdfTab) + kAdfWaves * sizeof(AdfList) + sizeof(unsigned) * ((size_t) nhist + kAdfCntWords); }

// Workgroups stride over the chunks of 256 places; within a chunk wave w takes the 64 places from 64 w, centre by centre.
// cosine: the ordinate is c over [-1, 1], scale = nbin / 2; otherwise the angle over [0, pi] (degrees and radians share their
// bins), scale = nbin / pi.
__global__ __launch_bounds__(256) void adf_hist_kernel(const Grid g, const int nall, const int nchunk, const int nbin,
                                                       const int ntriple, const int cosine, const double scale,
                                                       const double rmaxsq, const double4 *__restrict__ rec,
                                                       const int *__restrict__ cell_start, const unsigned *__restrict__ tab_g,
                                                       unsigned long long *__restrict__ hist, unsigned long long *__restrict__ cnt)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char adf_lds[];
  const int nhist = nbin * ntriple;
  const AdfTab *tab = (const AdfTab *) adf_lds;
  AdfList *lists = (AdfList *) (adf_lds + sizeof(AdfTab));
  unsigned *lh = (unsigned *) (adf_lds + sizeof(AdfTab) + kAdfWaves * sizeof(AdfList)), *lc = lh + nhist;
  for (int k = threadIdx.x; k < nhist + kAdfCntWords; k += 256) lh[k] = 0u;
  for (int k = threadIdx.x; k < kAdfTabWords; k += 256) ((unsigned *) adf_lds)[k] = tab_g[k];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  AdfList &L = lists[wave];
  int done = 0;
  for (int chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
    const int pi = chunk * 256 + threadIdx.x;
    int ci = 0;
    double4 xi = make_double4(0.0, 0.0, 0.0, 0.0);
    if (pi < nall) {
      xi = rec[pi];
      ci = __double2loint(xi.w);
    }
    const int ti = ci & (kBinTypes - 1);
    const unsigned cm = (ci & kBinOwned) && ti ? tab->imask[ti] : 0u; // the triples this owned member is a centre of
    for (unsigned m = cm; m; m &= m - 1) atomicAdd(lc + (__ffs(m) - 1), 1u);
    for (unsigned long long todo = __ballot(cm != 0u); todo; todo &= todo - 1) {
      const MdpWalkCentre ctr = mdp_walk_centre(todo, xi, (int) cm, chunk * 256 + wave * 64);
      const unsigned ccm = (unsigned) ctr.v;
      const int total = mdp_walk_runs(g, cell_start, ctr.x, lane, L.runs);
      int n = 0; // hits so far: the same in every lane
      for (int q0 = 0; q0 < total; q0 += 64) {
        MdpWalkCand c;
        const bool has = mdp_walk_cand(L.runs, q0 + lane, total, rec, ctr.x, c);
        bool hit = false;
        unsigned jm = 0u, km = 0u;
        if (has) {
          const int tj = __double2loint(c.xj.w) & (kBinTypes - 1);
          hit = tj && c.rsq < rmaxsq && c.p != ctr.p;
          if (hit) {
            for (unsigned m = tab->jmask[tj] & ccm; m; m &= m - 1) {
              const int k = __ffs(m) - 1;
              if (c.rsq >= tab->rsq[0][k] && c.rsq < tab->rsq[1][k]) jm |= 1u << k;
            }
            for (unsigned m = tab->kmask[tj] & ccm; m; m &= m - 1) {
              const int k = __ffs(m) - 1;
              if (c.rsq >= tab->rsq[2][k] && c.rsq < tab->rsq[3][k]) km |= 1u << k;
            }
          }
        }
        const int at = mdp_walk_slot(hit, lane, n);
        if (hit && at < MDP_ADF_MAXNEIGH) {
          L.dx[at] = c.dx;
          L.dy[at] = c.dy;
          L.dz[at] = c.dz;
          L.inv[at] = 1.0 / sqrt(c.rsq);
          L.jm[at] = jm;
          L.km[at] = km;
        }
      }
      mdp_wave_sync();
      if (n > MDP_ADF_MAXNEIGH) {
        if (lane == 0) atomicAdd(lc + MDP_ADF_MAXTRIPLE, 1u);
      } else if (n >= 2) {
        // q = a n + b over the n^2 ordered index pairs, 64 further per trip: one division per centre, none per trip
        const unsigned un = (unsigned) n, nn = un * un, da = 64u / un, db = 64u - da * un;
        unsigned a = (unsigned) lane / un, b = (unsigned) lane - a * un;
        for (unsigned q = (unsigned) lane; q < nn; q += 64u) {
          const unsigned m = L.jm[a] & L.km[b];
          if (m && a != b) {
            double c = (L.dx[a] * L.dx[b] + L.dy[a] * L.dy[b] + L.dz[a] * L.dz[b]) * (L.inv[a] * L.inv[b]);
            c = fmin(fmax(c, -1.0), 1.0);
            int bin = (int) ((cosine ? c + 1.0 : acos(c)) * scale);
            bin = bin < 0 ? 0 : (bin >= nbin ? nbin - 1 : bin);
            for (unsigned mm = m; mm; mm &= mm - 1) atomicAdd(lh + (__ffs(mm) - 1) * nbin + bin, 1u);
          }
          a += da;
          b += db;
          if (b >= un) {
            b -= un;
            a++;
          }
        }
      }
      mdp_wave_sync(); // the list is free for the wave's next centre
    }
    if (++done == kAdfChunksPerFlush) {
      mdp_lds_flush(lh, nhist, hist);
      done = 0;
    }
  }
  mdp_lds_flush(lh, nhist, hist);
  for (int k = threadIdx.x; k < kAdfCntWords - 1; k += 256)
    if (lc[k]) atomicAdd(cnt + k, (unsigned long long) lc[k]);
}

} // namespace

static void adf_release(mdp_ctx *c) // mdp_adf_off: the measurement's buffers go ahead of the context's end
{
  MdpAdf &h = c->adf;
  h.member.release();
  h.tab.release();
  h.bin.release();
  h.out.release();
  h.on = false;
}

extern "C" {

int mdp_adf_setup(mdp_ctx *c, int nbin, int ordinate, int ntriple, const int *ilo, const int *ihi, const int *jlo, const int *jhi,
                  const int *klo, const int *khi, const double *rjin, const double *rjout, const double *rkin, const double *rkout,
                  int ntag, const unsigned char *member_by_tag)
{
  MDP_TRY(mdp_measure_require(c, "mdp_adf_setup"));
  if (nbin < 1) return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: nbin must be >= 1, not %d", nbin);
  if (ordinate != MDP_ADF_DEGREE && ordinate != MDP_ADF_RADIAN && ordinate != MDP_ADF_COSINE)
    return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: ordinate must be 0 (degree), 1 (radian) or 2 (cosine), not %d", ordinate);
  if (ntriple < 1 || ntriple > MDP_ADF_MAXTRIPLE)
    return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: ntriple must be 1 .. %d, not %d", MDP_ADF_MAXTRIPLE, ntriple);
  if (!ilo || !ihi || !jlo || !jhi || !klo || !khi) return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: no type ranges");
  if (!rjin || !rjout || !rkin || !rkout) return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: no shell radii");
  int ntypes;
  MDP_TRY(mdp_measure_ntypes(c, "mdp_adf_setup", ntypes));
  double rmax = 0.0;
  for (int m = 0; m < ntriple; m++) {
    const int r[6] = {ilo[m], ihi[m], jlo[m], jhi[m], klo[m], khi[m]};
    MDP_TRY(mdp_measure_type_ranges(c, "mdp_adf_setup", "triple", m + 1, ntypes, 6, r));
    const double s[4] = {rjin[m], rjout[m], rkin[m], rkout[m]};
    for (int k = 0; k < 4; k++)
      if (!(s[k] >= 0.0) || !std::isfinite(s[k]))
        return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: triple %d: a radius must be >= 0, not %g", m + 1, s[k]);
    for (int k = 0; k < 4; k += 2)
      if (!(s[k] < s[k + 1]))
        return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: triple %d: the inner radius %g is not below the outer radius %g", m + 1, s[k], s[k + 1]);
    // the ghost shell and the skin, for the outer radius of either shell
    char what[40];
    snprintf(what, sizeof what, "triple %d: outer radius", m + 1);
    for (int k = 1; k < 4; k += 2) {
      MDP_TRY(mdp_measure_shell_setup(c, "mdp_adf_setup", what, "neighbours", s[k]));
      if (s[k] > rmax) rmax = s[k];
    }
  }
  if ((long long) nbin * ntriple > MDP_ADF_MAXCOUNTERS)
    return mdp_fail(c, MDP_EINVAL, "mdp_adf_setup: nbin x ntriple = %lld counters, the histogram in LDS holds %d", (long long) nbin * ntriple,
                    MDP_ADF_MAXCOUNTERS);
  MdpAdf &h = c->adf;
  MDP_TRY(mdp_measure_member(c, "mdp_adf_setup", ntag, member_by_tag, h.member, h.ntag));
  AdfTab tab = {};
  for (int m = 0; m < ntriple; m++) {
    tab.rsq[0][m] = rjin[m] * rjin[m];
    tab.rsq[1][m] = rjout[m] * rjout[m];
    tab.rsq[2][m] = rkin[m] * rkin[m];
    tab.rsq[3][m] = rkout[m] * rkout[m];
    for (int t = ilo[m]; t <= ihi[m]; t++) tab.imask[t] |= 1u << m;
    for (int t = jlo[m]; t <= jhi[m]; t++) tab.jmask[t] |= 1u << m;
    for (int t = klo[m]; t <= khi[m]; t++) tab.kmask[t] |= 1u << m;
  }
  MDP_HIP(c, h.tab.reserve(sizeof(AdfTab) / sizeof(double)));
  MDP_HIP(c, h.out.reserve((size_t) nbin * ntriple + kAdfCntWords));
  MDP_TRY(mdp_write_small(c, h.tab.p, &tab, sizeof tab));
  h.nbin = nbin;
  h.ntriple = ntriple;
  h.ntypes = ntypes;
  h.ordinate = ordinate;
  h.rmax = rmax;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_adf_counts(mdp_ctx *c, long long *hist, long long *icount)
{
  MDP_TRY(mdp_measure_require(c, "mdp_adf_counts"));
  if (!hist || !icount) return MDP_EINVAL;
  MdpAdf &h = c->adf;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_adf_setup not called");
  hipStream_t st = c->stream;
  const int nall = c->nall, nhist = h.nbin * h.ntriple, nout = nhist + kAdfCntWords;
  unsigned long long *d_hist = h.out.p, *d_cnt = h.out.p + nhist;
  MDP_TRY(mdp_hist_open(c, "mdp_adf_counts", "largest outer radius", h.rmax, "mdp_adf_setup", h.out.p, nout));
  if (nall > 0 && c->nlocal > 0) {
    Grid g;
    MDP_TRY(mdp_measure_bin(c, h.bin, h.rmax, h.ntypes, h.ntag, h.member.p, d_cnt + kAdfCntWords - 1, g));
    const int nchunk = nblk(nall);
    const size_t lds = adf_lds_bytes(nhist);
    int resident;
    MDP_TRY(mdp_measure_resident(c, lds, resident));
    const int grid = mdp_measure_grid(nchunk, resident);
    const int cosine = h.ordinate == MDP_ADF_COSINE;
    adf_hist_kernel<<<grid, 256, lds, st>>>(g, nall, nchunk, h.nbin, h.ntriple, cosine, cosine ? 0.5 * h.nbin : h.nbin / M_PI,
                                            h.rmax * h.rmax, h.bin.rec.p, h.bin.cell_start.p, (const unsigned *) h.tab.p, d_hist, d_cnt);
    MDP_HIP(c, hipGetLastError());
  }
  std::vector<unsigned long long> host;
  MDP_TRY(mdp_hist_download(c, "mdp_adf_counts", "mdp_adf_setup", h.out.p, nout, h.ntag, host));
  const unsigned long long *cnt = host.data() + nhist;
  if (cnt[MDP_ADF_MAXTRIPLE])
    return mdp_fail(c, MDP_EINVAL, "mdp_adf_counts: %lld centres have more than %d neighbours inside the largest outer radius %g, the short "
                                   "list of a wave: use smaller outer radii",
                    (long long) cnt[MDP_ADF_MAXTRIPLE], MDP_ADF_MAXNEIGH, h.rmax);
  for (int k = 0; k < nhist; k++) hist[k] = (long long) host[k];
  for (int m = 0; m < h.ntriple; m++) icount[m] = (long long) cnt[m];
  return MDP_OK;
}

int mdp_adf_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->adf, c->adf.nbin, c->adf.ntriple, out);
}

int mdp_adf_off(mdp_ctx *c) { return mdp_measure_off(c, adf_release); }

} // extern "C"
