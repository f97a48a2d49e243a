/* ------------------------------------------------------------------------------------------------
   compute rdf/mdp -- see compute_rdf_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: Nbin < 1, an odd number of type
                        arguments, a type outside 1 .. ntypes, an unknown keyword, a cutoff without a value or <= 0,
                        more than 32 pairs, more counters than the device's histogram holds)
     init()             bricks mode (the host-linked mode: there the host's atom->x is current, and compute rdf is right);
                        the cutoff against the pair style's cutforce; the member table from atom->mask at this rank's
                        tags, made whole over the ranks
     compute_array()    the setup goes up once per context and run (mdp_rdf_setup); mdp_rdf_counts on this rank's brick,
                        the counts summed over the ranks (sum_whole), LAMMPS' normalisation
   The group refusals, the integrator, the run's context, the once-per-context protocol and the exact sum: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_rdf_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "pair.h"
#include "update.h"

#include <cmath>
#include <string>

using namespace LAMMPS_NS;

ComputeRDFMDP::ComputeRDFMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "rdf/mdp", "there is no pair to count"), nbin(0), npairs(0), cutflag(0), cutoff_user(0.0), cutoff(0.0)
{
  if (narg < 4) error->all(FLERR, head + "compute ID GROUP rdf/mdp Nbin [itype jtype ...] [cutoff Rc]");
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
        if (!mdp_type_bounds(a, ntypes, s ? jlo[m] : ilo[m], s ? jhi[m] : ihi[m]))
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

  global_array(nbin, 1 + 2 * npairs);
}

ComputeRDFMDP::~ComputeRDFMDP() {}

void ComputeRDFMDP::init()
{
  require_bricks("where the host's atom->x and neighbour list are current: use compute rdf (or run the fix with bricks yes)");
  if (!force->pair) error->all(FLERR, "Compute rdf/mdp requires a pair style: its cutforce sets the ghost shell the partners come from");
  const double cutforce = force->pair->cutforce;
  cutoff = cutflag ? cutoff_user : cutforce;
  if (cutoff > cutforce * (1.0 + 1e-12)) {
    char buf[256];
    snprintf(buf, sizeof buf, "Compute rdf/mdp: cutoff %g is beyond the pair style's cutforce %.15g: the brick's ghost shell is cutforce + skin wide as of "
                              "the last reneighbouring, so only pairs within cutforce are all present", cutoff, cutforce);
    error->all(FLERR, buf);
  }
  // Membership by tag for the whole system: each rank marks its own atoms and the table is made whole over the ranks --
  // every tag is owned by one rank, and the sum of its marks is its maximum.  Group all: no table.
  member.clear();
  forget(); // a new init() may bring a new group membership: the setup goes up again
  if (igroup > 0) {
    const bigint n = atom->natoms;
    member.assign((size_t) n, 0);
    for (int i = 0; i < atom->nlocal; i++) {
      const bigint t = atom->tag[i];
      if (t < 1 || t > n) error->one(FLERR, "Compute rdf/mdp requires consecutive atom IDs 1 .. natoms");
      if (atom->mask[i] & groupbit) member[(size_t) (t - 1)] = 1;
    }
    sum_whole(member.data(), member.size());
  }
}

void ComputeRDFMDP::compute_array()
{
  invoked_array = update->ntimestep;
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_rdf_info)) {
    if (mdp_rdf_setup(c, nbin, cutoff, npairs, ilo.data(), ihi.data(), jlo.data(), jhi.data(), (int) member.size(),
                      member.empty() ? nullptr : member.data()) != MDP_OK)
      fail(c);
    record(c, mdp_rdf_info);
  }
  const size_t nh = (size_t) nbin * npairs, nw = nh + 3 * (size_t) npairs;
  std::vector<long long> cnt(nw, 0);
  if (mdp_rdf_counts(c, cnt.data(), cnt.data() + nh, cnt.data() + nh + npairs, cnt.data() + nh + 2 * npairs) != MDP_OK) fail(c);
  sum_whole(cnt.data(), nw);
  const std::vector<double> tot(cnt.begin(), cnt.end());
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
