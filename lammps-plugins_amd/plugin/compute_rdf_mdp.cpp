/* ------------------------------------------------------------------------------------------------
   compute rdf/mdp -- see compute_rdf_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: Nbin < 1, an odd number of type
                        arguments, a type outside 1 .. ntypes, an unknown keyword, a cutoff without a value or <= 0, an
                        unknown or empty group, more than 32 pairs, more counters than the device's histogram holds)
     init()             the one fix nve/mdp (or nvt/mdp) found through modify, in bricks mode (refused: none, the
                        host-linked mode -- there the host's atom->x is current, and compute rdf is right); the cutoff
                        against the pair style's cutforce; the member table from atom->mask at this rank's tags, made
                        whole over the ranks
     compute_array()    the run's context through Fix::extract("mdp_steps_ctx"); the setup goes up once per context
                        (mdp_rdf_setup; mdp_rdf_info tells whether it is still there); mdp_rdf_counts on this rank's
                        brick, the counts summed over the ranks (as doubles: exact below 2^53), LAMMPS' normalisation
-------------------------------------------------------------------------------------------------- */
#include "compute_rdf_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "fix.h"
#include "force.h"
#include "group.h"
#include "modify.h"
#include "pair.h"
#include "update.h"

#include <cmath>
#include <cstring>
#include <string>

using namespace LAMMPS_NS;

namespace {
// a LAMMPS type argument N, *, N*, *M or N*M over 1 .. ntypes (utils::bounds)
bool type_bounds(const std::string &s, const int ntypes, int &lo, int &hi)
{
  const size_t star = s.find('*');
  long long a = 0, b = 0;
  if (star == std::string::npos) {
    if (!mdp_whole(s.c_str(), a)) return false;
    b = a;
  } else {
    const std::string l = s.substr(0, star), r = s.substr(star + 1);
    if (r.find('*') != std::string::npos) return false;
    a = 1;
    b = ntypes;
    if (!l.empty() && !mdp_whole(l.c_str(), a)) return false;
    if (!r.empty() && !mdp_whole(r.c_str(), b)) return false;
  }
  if (a < 1 || b > ntypes || a > b) return false;
  lo = (int) a;
  hi = (int) b;
  return true;
}
}    // namespace

ComputeRDFMDP::ComputeRDFMDP(LAMMPS *lmp, int narg, char **arg)
    : Compute(lmp, narg, arg), nbin(0), npairs(0), cutflag(0), cutoff_user(0.0), cutoff(0.0), sent_to(nullptr), sent_serial(0)
{
  const std::string head = "Illegal compute rdf/mdp command: ";
  if (narg < 4) error->all(FLERR, head + "compute ID GROUP rdf/mdp Nbin [itype jtype ...] [cutoff Rc]");
  if (igroup < 0)
    error->all(FLERR, std::string("Compute rdf/mdp requires group all or a group defined by the group command: could not find compute group ID ") + arg[1]);
  if (igroup > 0 && group->count(igroup) == 0)
    error->all(FLERR, std::string("Compute rdf/mdp: group ") + arg[1] + " is empty: there is no pair to count");
  long long nb = 0;
  if (!mdp_whole(arg[3], nb) || nb < 1 || nb > 2147483647) error->all(FLERR, head + "Nbin must be a whole number >= 1, not " + arg[3]);
  nbin = (int) nb;
  // type arguments up to the first keyword; keywords behind them
  int iarg = 4;
  while (iarg < narg && (isdigit((unsigned char) arg[iarg][0]) || arg[iarg][0] == '*' || arg[iarg][0] == '-')) iarg++;
  const int ntype_args = iarg - 4;
  if (ntype_args % 2) error->all(FLERR, head + "the type arguments come in pairs itype jtype, and there are " + std::to_string(ntype_args));
  const int ntypes = atom->ntypes;
  if (ntype_args == 0) {
    npairs = 1;
    ilo.assign(1, 1);
    ihi.assign(1, ntypes);
    jlo.assign(1, 1);
    jhi.assign(1, ntypes);
  } else {
    npairs = ntype_args / 2;
    if (npairs > MDP_RDF_MAXPAIR) error->all(FLERR, head + std::to_string(npairs) + " type pairs; at most " + std::to_string(MDP_RDF_MAXPAIR) + " fit one compute");
    ilo.resize(npairs);
    ihi.resize(npairs);
    jlo.resize(npairs);
    jhi.resize(npairs);
    for (int m = 0; m < npairs; m++)
      for (int s = 0; s < 2; s++) {
        const char *a = arg[4 + 2 * m + s];
        if (!type_bounds(a, ntypes, s ? jlo[m] : ilo[m], s ? jhi[m] : ihi[m]))
          error->all(FLERR, head + "type " + a + " is not N, *, N*, *M or N*M within 1 .. " + std::to_string(ntypes));
      }
  }
  while (iarg < narg) {
    const std::string key = arg[iarg];
    if (key != "cutoff") error->all(FLERR, head + "unknown keyword " + key);
    if (iarg + 1 >= narg) error->all(FLERR, head + "cutoff needs a value");
    cutoff_user = mdp_number(error, head, "cutoff", arg[iarg + 1], true);
    if (!(cutoff_user > 0.0)) error->all(FLERR, head + "cutoff must be > 0, not " + arg[iarg + 1]);
    cutflag = 1;
    iarg += 2;
  }
  if ((long long) nbin * npairs > MDP_RDF_MAXCOUNTERS)
    error->all(FLERR, head + std::to_string(nbin) + " bins x " + std::to_string(npairs) + " pairs; the device's histogram holds " +
                          std::to_string(MDP_RDF_MAXCOUNTERS) + " counters");
  if (atom->natoms < 1) error->all(FLERR, "Compute rdf/mdp: there are no atoms");
  if (!atom->tag_enable) error->all(FLERR, "Compute rdf/mdp requires atom IDs");

  array_flag = 1;
  extarray = 0;
  size_array_rows = nbin;
  size_array_cols = 1 + 2 * npairs;
  values.assign((size_t) nbin * size_array_cols, 0.0);
  rows.resize(nbin);
  for (int b = 0; b < nbin; b++) rows[b] = values.data() + (size_t) b * size_array_cols;
  array = rows.data();
}

ComputeRDFMDP::~ComputeRDFMDP() {}

void ComputeRDFMDP::fail(mdp_ctx *c) { error->one(FLERR, std::string("Compute rdf/mdp: ") + (c ? mdp_last_error(c) : "no device context")); }

// the one time integrator of this plugin family: fix nve/mdp, or fix nvt/mdp that is built on it
Fix *ComputeRDFMDP::integrator() const
{
  Fix *found = nullptr;
  for (int i = 0; i < modify->nfix; i++) {
    Fix *f = modify->fix[i];
    if (strcmp(f->style, "nve/mdp") != 0 && strcmp(f->style, "nvt/mdp") != 0) continue;
    if (found) error->all(FLERR, std::string("Compute rdf/mdp: fixes ") + found->id + " and " + f->id + " both integrate on the device; it reads one run's context");
    found = f;
  }
  return found;
}

void ComputeRDFMDP::init()
{
  Fix *nve = integrator();
  if (!nve) error->all(FLERR, "Compute rdf/mdp requires fix nve/mdp (or fix nvt/mdp) with bricks yes as the time integrator");
  int dim = 0;
  const int *bricks = static_cast<int *>(nve->extract("mdp_bricks", dim));
  if (!bricks || !nve->extract("mdp_steps_ctx", dim)) error->all(FLERR, std::string("Compute rdf/mdp: fix ") + nve->id + " does not expose its run's context");
  if (!*bricks)
    error->all(FLERR, std::string("Compute rdf/mdp: fix ") + nve->id + " runs in the host-linked mode, where the host's atom->x and neighbour list are current: use compute rdf (or run the fix with bricks yes)");
  if (!force->pair) error->all(FLERR, "Compute rdf/mdp requires a pair style: its cutforce sets the ghost shell the partners come from");
  const double cutforce = force->pair->cutforce;
  cutoff = cutflag ? cutoff_user : cutforce;
  if (cutoff > cutforce * (1.0 + 1e-12)) {
    char buf[256];
    snprintf(buf, sizeof buf, "Compute rdf/mdp: cutoff %g is beyond the pair style's cutforce %.15g: the brick's ghost shell is cutforce + skin wide as of "
                              "the last reneighbouring, so only pairs within cutforce are all present", cutoff, cutforce);
    error->all(FLERR, buf);
  }
  // Membership by tag for the whole system: each rank marks its own atoms and the table is made whole over the ranks.
  // The mini-host's MPI subset has one reduction, MPI_SUM of MPI_DOUBLE (lammps_host_api.h: no byte or int types, no
  // MPI_MAX), so the marks travel as doubles -- every tag is owned by one rank, and the sum of its marks is its maximum --
  // in pieces of 64 K tags: 1 MB of transient buffers whatever the size of the system.  Group all: no table.
  member.clear();
  sent_to = nullptr; // a new init() may bring a new group membership: the setup goes up again
  if (igroup > 0) {
    const bigint n = atom->natoms;
    member.assign((size_t) n, 0);
    for (int i = 0; i < atom->nlocal; i++) {
      const bigint t = atom->tag[i];
      if (t < 1 || t > n) error->one(FLERR, "Compute rdf/mdp requires consecutive atom IDs 1 .. natoms");
      if (atom->mask[i] & groupbit) member[(size_t) (t - 1)] = 1;
    }
    const bigint piece = 65536;
    std::vector<double> mine((size_t) piece), all((size_t) piece);
    for (bigint t0 = 0; t0 < n; t0 += piece) {
      const int len = (int) (n - t0 < piece ? n - t0 : piece);
      for (int k = 0; k < len; k++) mine[k] = member[(size_t) (t0 + k)] ? 1.0 : 0.0;
      MPI_Allreduce(mine.data(), all.data(), len, MPI_DOUBLE, MPI_SUM, world);
      for (int k = 0; k < len; k++) member[(size_t) (t0 + k)] = all[k] > 0.0 ? 1 : 0;
    }
  }
}

void ComputeRDFMDP::compute_array()
{
  invoked_array = update->ntimestep;
  Fix *nve = integrator();
  int dim = 0;
  mdp_ctx **slot = nve ? static_cast<mdp_ctx **>(nve->extract("mdp_steps_ctx", dim)) : nullptr;
  mdp_ctx *c = slot ? *slot : nullptr;
  if (!c) error->all(FLERR, "Compute rdf/mdp: no run of fix nve/mdp is under way; the atoms are on the device only during one");
  long long info[4] = {0, 0, 0, 0};
  if (mdp_rdf_info(c, info) != MDP_OK) fail(c);
  if (c != sent_to || !info[0] || info[3] != sent_serial) { // once per context, unless another measurement took its place
    if (mdp_rdf_setup(c, nbin, cutoff, npairs, ilo.data(), ihi.data(), jlo.data(), jhi.data(), (int) member.size(),
                      member.empty() ? nullptr : member.data()) != MDP_OK)
      fail(c);
    if (mdp_rdf_info(c, info) != MDP_OK) fail(c);
    sent_to = c;
    sent_serial = info[3];
  }
  const size_t nh = (size_t) nbin * npairs, nw = nh + 3 * (size_t) npairs;
  std::vector<long long> cnt(nw, 0);
  if (mdp_rdf_counts(c, cnt.data(), cnt.data() + nh, cnt.data() + nh + npairs, cnt.data() + nh + 2 * npairs) != MDP_OK) fail(c);
  std::vector<double> mine(nw), tot(nw);
  for (size_t k = 0; k < nw; k++) mine[k] = (double) cnt[k];
  MPI_Allreduce(mine.data(), tot.data(), (int) nw, MPI_DOUBLE, MPI_SUM, world);
  const double *hist = tot.data(), *icount = hist + nh, *jcount = icount + npairs, *dup = jcount + npairs;

  // LAMMPS' ComputeRDF::compute_array: g = hist / (vfrac normfac icount), coord = running sum of g vfrac normfac
  const double delr = cutoff / nbin;
  const double constant = 4.0 * M_PI / (3.0 * domain->xprd * domain->yprd * domain->zprd);
  for (int b = 0; b < nbin; b++) array[b][0] = (b + 0.5) * delr;
  for (int m = 0; m < npairs; m++) {
    const double normfac = icount[m] > 0.0 ? jcount[m] - dup[m] / icount[m] : 0.0;
    double ncoord = 0.0;
    for (int b = 0; b < nbin; b++) {
      const double rlower = b * delr, rupper = (b + 1) * delr;
      const double vfrac = constant * (rupper * rupper * rupper - rlower * rlower * rlower);
      const double gr = vfrac * normfac * icount[m] != 0.0 ? hist[(size_t) m * nbin + b] / (vfrac * normfac * icount[m]) : 0.0;
      ncoord += gr * vfrac * normfac;
      array[b][1 + 2 * m] = gr;
      array[b][2 + 2 * m] = ncoord;
    }
  }
}
