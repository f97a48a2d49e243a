// rdf.hip -- pair-distance histograms of a device-resident run (LAMMPS compute rdf), in integers.
// A read bins ALL atoms of the brick (owned and ghost) on a grid of its own, at cell width >= cutoff / 2, into buffers that
// belong to MdpRdf (mdp_measure_bin, measure_bin.hip, which compute adf's read shares): the list builders' grid,
// permutation, cell starts and cell-ordered positions (mdp_bin_atoms) are
// neither read nor written, so a read changes nothing a later step or list build sees.  One lane per atom in cell order
// (a wave shares its 5 x 5 x 5 stencil) sweeps the stencil as 25 runs of the cell-ordered records {x, y, z, code}; the
// code word carries the type (0 for an atom outside the group), so one 32-byte load per candidate is all the inner loop
// reads.  Hits go into a per-workgroup LDS histogram of 32-bit counters (LDS integer atomics); its non-zero counters
// are added to the global 64-bit histogram with device-scope integer atomics.  No floating-point atomic anywhere:
// two reads of one state agree exactly, and the sum over the bricks of a decomposition is the one-brick histogram.
#include "measure_walk.h"

namespace {

constexpr int kRdfTypes = kBinTypes;   // type codes 0 .. 15: 0 = not a member, t = LAMMPS type t
constexpr int kRdfOwned = kBinOwned;   // code bit: an owned atom (a lane that counts)
constexpr int kRdfTabWords = kRdfTypes * kRdfTypes + 2 * kRdfTypes; // column masks per (ti, tj), then i masks, j masks per type
constexpr int kRdfChunksPerFlush = 64; // a workgroup flushes its 32-bit counters after this many chunks of 256 atoms:
                                       // no counter overflows below 2^32 / (64 * 256) = 262 144 candidates per atom
constexpr int kRdfCntWords = 3 * MDP_RDF_MAXPAIR + 1; // icount, jcount, dup per column, then the atoms whose tag has no entry

using Grid = MdpGrid;

// Dynamic LDS, in 32-bit words: [0, nhist) the histogram [column][bin], [nhist, nhist + kRdfCntWords) icount / jcount /
// dup, then the kRdfTabWords mask table.  Workgroups stride over the chunks of 256 places, so that a workgroup's
// counters are flushed once per kRdfChunksPerFlush chunks and not once per chunk.
__global__ __launch_bounds__(256) void rdf_hist_kernel(const Grid g, const int nall, const int nchunk, const int nbin,
                                                       const int npair, const double scale, const double cutsq_hi,
                                                       const double4 *__restrict__ rec, const int *__restrict__ cell_start,
                                                       const int *__restrict__ tab_g, unsigned long long *__restrict__ hist,
                                                       unsigned long long *__restrict__ cnt)
{
  extern __shared__ __attribute__((aligned(16))) unsigned rdf_lds[];
  const int nhist = nbin * npair;
  unsigned *lh = rdf_lds, *lc = rdf_lds + nhist;
  int *tab = (int *) (rdf_lds + nhist + kRdfCntWords);
  for (int k = threadIdx.x; k < nhist + kRdfCntWords; k += 256) rdf_lds[k] = 0u;
  for (int k = threadIdx.x; k < kRdfTabWords; k += 256) tab[k] = tab_g[k];
  __syncthreads();
  int done = 0;
  for (int chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
    const int pi = chunk * 256 + threadIdx.x;
    int ci = 0;
    double4 xi = make_double4(0.0, 0.0, 0.0, 0.0);
    if (pi < nall) {
      xi = rec[pi];
      ci = __double2loint(xi.w);
    }
    const int ti = ci & (kRdfTypes - 1);
    if ((ci & kRdfOwned) && ti) { // an owned member
      const unsigned im = (unsigned) tab[kRdfTypes * kRdfTypes + ti], jm = (unsigned) tab[kRdfTypes * kRdfTypes + kRdfTypes + ti];
      for (unsigned m = im; m; m &= m - 1) atomicAdd(lc + (__ffs(m) - 1), 1u);
      for (unsigned m = jm; m; m &= m - 1) atomicAdd(lc + MDP_RDF_MAXPAIR + (__ffs(m) - 1), 1u);
      for (unsigned m = im & jm; m; m &= m - 1) atomicAdd(lc + 2 * MDP_RDF_MAXPAIR + (__ffs(m) - 1), 1u);
      if (im) {
        const int *row = tab + kRdfTypes * ti;
        int cx, cy, cz;
        mdp_bin_cell_index(g, xi, cx, cy, cz);
        const int x0 = max(cx - 2, 0), x1 = min(cx + 2, g.n[0] - 1);
        for (int z = max(cz - 2, 0); z <= min(cz + 2, g.n[2] - 1); z++)
          for (int y = max(cy - 2, 0); y <= min(cy + 2, g.n[1] - 1); y++) {
            const int c0 = g.n[0] * (y + g.n[1] * z);
            const int pb = cell_start[c0 + x0], pe = cell_start[c0 + x1 + 1]; // cells along x are contiguous in the sort
            for (int p = pb; p < pe; p++) {
              const double4 xj = rec[p];
              const double dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
              const double rsq = dx * dx + dy * dy + dz * dz;
              if (rsq < cutsq_hi && p != pi) {
                const unsigned cols = (unsigned) row[__double2loint(xj.w) & (kRdfTypes - 1)];
                if (cols) {
                  const int b = (int) (sqrt(rsq) * scale);
                  if (b < nbin)
                    for (unsigned m = cols; m; m &= m - 1) atomicAdd(lh + (__ffs(m) - 1) * nbin + b, 1u);
                }
              }
            }
          }
      }
    }
    if (++done == kRdfChunksPerFlush) {
      mdp_lds_flush(lh, nhist, hist);
      done = 0;
    }
  }
  mdp_lds_flush(lh, nhist, hist);
  for (int k = threadIdx.x; k < kRdfCntWords - 1; k += 256)
    if (lc[k]) atomicAdd(cnt + k, (unsigned long long) lc[k]);
}

} // namespace

static void rdf_release(mdp_ctx *c) // mdp_rdf_off: the measurement's buffers go ahead of the context's end
{
  MdpRdf &h = c->rdf;
  h.member.release();
  h.tab.release();
  h.bin.release();
  h.out.release();
  h.on = false;
}

extern "C" {

int mdp_rdf_setup(mdp_ctx *c, int nbin, double cutoff, int npair, const int *ilo, const int *ihi, const int *jlo,
                  const int *jhi, int ntag, const unsigned char *member_by_tag)
{
  MDP_TRY(mdp_measure_require(c, "mdp_rdf_setup"));
  if (nbin < 1) return mdp_fail(c, MDP_EINVAL, "mdp_rdf_setup: nbin must be >= 1, not %d", nbin);
  if (npair < 1 || npair > MDP_RDF_MAXPAIR)
    return mdp_fail(c, MDP_EINVAL, "mdp_rdf_setup: npair must be 1 .. %d, not %d", MDP_RDF_MAXPAIR, npair);
  if (!ilo || !ihi || !jlo || !jhi) return mdp_fail(c, MDP_EINVAL, "mdp_rdf_setup: no type ranges");
  int ntypes;
  MDP_TRY(mdp_measure_ntypes(c, "mdp_rdf_setup", ntypes));
  for (int m = 0; m < npair; m++) {
    const int r[4] = {ilo[m], ihi[m], jlo[m], jhi[m]};
    MDP_TRY(mdp_measure_type_ranges(c, "mdp_rdf_setup", "pair", m + 1, ntypes, 4, r));
  }
  if (!(cutoff > 0.0)) return mdp_fail(c, MDP_EINVAL, "mdp_rdf_setup: cutoff must be > 0, not %g", cutoff);
  MDP_TRY(mdp_measure_shell_setup(c, "mdp_rdf_setup", "cutoff", "pairs", cutoff));
  if ((long long) nbin * npair > MDP_RDF_MAXCOUNTERS)
    return mdp_fail(c, MDP_EINVAL, "mdp_rdf_setup: nbin x npair = %lld counters, the histogram in LDS holds %d", (long long) nbin * npair,
                    MDP_RDF_MAXCOUNTERS);
  MdpRdf &h = c->rdf;
  MDP_TRY(mdp_measure_member(c, "mdp_rdf_setup", ntag, member_by_tag, h.member, h.ntag));
  int tab[kRdfTabWords] = {};
  for (int m = 0; m < npair; m++) {
    for (int ti = ilo[m]; ti <= ihi[m]; ti++) {
      tab[kRdfTypes * kRdfTypes + ti] |= (int) (1u << m);
      for (int tj = jlo[m]; tj <= jhi[m]; tj++) tab[kRdfTypes * ti + tj] |= (int) (1u << m);
    }
    for (int tj = jlo[m]; tj <= jhi[m]; tj++) tab[kRdfTypes * kRdfTypes + kRdfTypes + tj] |= (int) (1u << m);
  }
  MDP_HIP(c, h.tab.reserve(kRdfTabWords));
  MDP_HIP(c, h.out.reserve((size_t) nbin * npair + kRdfCntWords));
  MDP_TRY(mdp_write_small(c, h.tab.p, tab, sizeof tab));
  h.nbin = nbin;
  h.npair = npair;
  h.ntypes = ntypes;
  h.cutoff = cutoff;
  mdp_measure_start(h);
  return MDP_OK;
}

int mdp_rdf_counts(mdp_ctx *c, long long *hist, long long *icount, long long *jcount, long long *dup)
{
  MDP_TRY(mdp_measure_require(c, "mdp_rdf_counts"));
  if (!hist || !icount || !jcount || !dup) return MDP_EINVAL;
  MdpRdf &h = c->rdf;
  if (!h.on) return mdp_fail(c, MDP_ESTATE, "mdp_rdf_setup not called");
  hipStream_t st = c->stream;
  const int nall = c->nall, nhist = h.nbin * h.npair, nout = nhist + kRdfCntWords;
  unsigned long long *d_hist = h.out.p, *d_cnt = h.out.p + nhist;
  MDP_TRY(mdp_hist_open(c, "mdp_rdf_counts", "cutoff", h.cutoff, "mdp_rdf_setup", h.out.p, nout));
  if (nall > 0 && c->nlocal > 0) {
    Grid g;
    MDP_TRY(mdp_measure_bin(c, h.bin, h.cutoff, h.ntypes, h.ntag, h.member.p, d_cnt + kRdfCntWords - 1, g));
    const int nchunk = nblk(nall);
    const size_t lds = sizeof(unsigned) * ((size_t) nhist + kRdfCntWords + kRdfTabWords);
    int resident;
    MDP_TRY(mdp_measure_resident(c, lds, resident));
    const int grid = mdp_measure_grid(nchunk, resident);
    // every pair with (int) (r nbin / cutoff) < nbin has rsq below this; the bin index decides
    const double cutsq_hi = h.cutoff * h.cutoff * (1.0 + 1e-9);
    rdf_hist_kernel<<<grid, 256, lds, st>>>(g, nall, nchunk, h.nbin, h.npair, (double) h.nbin / h.cutoff, cutsq_hi, h.bin.rec.p,
                                            h.bin.cell_start.p, h.tab.p, d_hist, d_cnt);
    MDP_HIP(c, hipGetLastError());
  }
  std::vector<unsigned long long> host;
  MDP_TRY(mdp_hist_download(c, "mdp_rdf_counts", "mdp_rdf_setup", h.out.p, nout, h.ntag, host));
  const unsigned long long *cnt = host.data() + nhist;
  for (int k = 0; k < nhist; k++) hist[k] = (long long) host[k];
  for (int m = 0; m < h.npair; m++) {
    icount[m] = (long long) cnt[m];
    jcount[m] = (long long) cnt[MDP_RDF_MAXPAIR + m];
    dup[m] = (long long) cnt[2 * MDP_RDF_MAXPAIR + m];
  }
  return MDP_OK;
}

int mdp_rdf_info(mdp_ctx *c, long long out[4])
{
  if (!c || !out) return MDP_EINVAL;
  return mdp_measure_info(c->rdf, c->rdf.nbin, c->rdf.npair, out);
}

int mdp_rdf_off(mdp_ctx *c) { return mdp_measure_off(c, rdf_release); }

} // extern "C"
