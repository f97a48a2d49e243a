/* ------------------------------------------------------------------------------------------------
   compute adf/mdp -- see compute_adf_mdp.h.  What runs where:
     constructor        the arguments, before any device is touched (refused here: Nbin < 1, a number of triple arguments
                        that is no multiple of 7, a type outside 1 .. ntypes, a bad or negative radius, inner >= outer,
                        more than 32 triples, more counters than the device's histogram holds, an unknown keyword or value)
     init()             bricks mode (the host-linked mode: there the host's atom->x is current, and compute adf is right);
                        the outer radii against the pair style's cutforce; the member table from atom->mask at this rank's
                        tags, made whole over the ranks
     compute_array()    the setup goes up once per context and run (mdp_adf_setup); mdp_adf_counts on this rank's brick,
                        the counts summed over the ranks (sum_whole), the normalisation
   The group refusals, the integrator, the run's context, the once-per-context protocol and the exact sum: compute_mdp.h.
-------------------------------------------------------------------------------------------------- */
#include "compute_adf_mdp.h"
#include "mdp_args.h"

#include "atom.h"
#include "comm.h"
#include "error.h"
#include "force.h"
#include "pair.h"
#include "update.h"

#include <cmath>
#include <string>

using namespace LAMMPS_NS;

ComputeADFMDP::ComputeADFMDP(LAMMPS *lmp, int narg, char **arg)
    : ComputeMDP(lmp, narg, arg, "adf/mdp", "there is no angle to count"), nbin(0), ntriples(0), ordinate(MDP_ADF_DEGREE), per_centre(0),
      default_shells(false)
{
  if (narg < 4)
    error->all(FLERR, head + "compute ID GROUP adf/mdp Nbin [itype jtype ktype Rjinner Rjouter Rkinner Rkouter ...] [ordinate degree|radian|cosine] "
                             "[cumulative fraction|centre]");
  long long nb = 0;
  if (!mdp_whole(arg[3], nb) || nb < 1 || nb > 2147483647) error->all(FLERR, head + "Nbin must be a whole number >= 1, not " + arg[3]);
  nbin = (int) nb;
  // triple arguments up to the first keyword; keywords behind them
  int iarg = 4;
  while (iarg < narg && (isdigit((unsigned char) arg[iarg][0]) || (arg[iarg][0] && strchr("*-+.", arg[iarg][0])))) iarg++;
  const int ntriple_args = iarg - 4;
  if (ntriple_args % 7)
    error->all(FLERR, head + "the triple arguments come in sevens itype jtype ktype Rjinner Rjouter Rkinner Rkouter, and there are " +
                          std::to_string(ntriple_args));
  const int ntypes = atom->ntypes;
  default_shells = ntriple_args == 0;
  ntriples = default_shells ? 1 : ntriple_args / 7;
  if (ntriples > MDP_ADF_MAXTRIPLE)
    error->all(FLERR, head + std::to_string(ntriples) + " triples; at most " + std::to_string(MDP_ADF_MAXTRIPLE) + " fit one compute");
  ilo.assign(ntriples, 1);
  jlo = klo = ilo;
  ihi.assign(ntriples, ntypes);
  jhi = khi = ihi;
  rjin.assign(ntriples, 0.0);
  rjout = rkin = rkout = rjin;
  for (int m = 0; m < ntriples && !default_shells; m++) {
    char **a = arg + 4 + 7 * m;
    int *lo[3] = {&ilo[m], &jlo[m], &klo[m]}, *hi[3] = {&ihi[m], &jhi[m], &khi[m]};
    for (int s = 0; s < 3; s++)
      if (!mdp_type_bounds(a[s], ntypes, *lo[s], *hi[s]))
        error->all(FLERR, head + "type " + a[s] + " is not N, *, N*, *M or N*M within 1 .. " + std::to_string(ntypes));
    double *r[4] = {&rjin[m], &rjout[m], &rkin[m], &rkout[m]};
    for (int s = 0; s < 4; s++) {
      *r[s] = mdp_number(error, head, "radius", a[3 + s], true);
      if (*r[s] < 0.0) error->all(FLERR, head + "a radius must be >= 0, not " + a[3 + s]);
    }
    for (int s = 0; s < 4; s += 2)
      if (!(*r[s] < *r[s + 1]))
        error->all(FLERR, head + "triple " + std::to_string(m + 1) + ": the inner radius " + a[3 + s] + " is not below the outer radius " + a[4 + s]);
  }
  while (iarg < narg) {
    const std::string key = arg[iarg];
    if (key != "ordinate" && key != "cumulative") error->all(FLERR, head + "unknown keyword " + key);
    if (iarg + 1 >= narg) error->all(FLERR, head + key + " needs a value");
    const std::string val = arg[iarg + 1];
    if (key == "ordinate") {
      if (val == "degree") ordinate = MDP_ADF_DEGREE;
      else if (val == "radian") ordinate = MDP_ADF_RADIAN;
      else if (val == "cosine") ordinate = MDP_ADF_COSINE;
      else error->all(FLERR, head + "ordinate takes degree, radian or cosine, not " + val);
    } else {
      if (val != "fraction" && val != "centre") error->all(FLERR, head + "cumulative takes fraction or centre, not " + val);
      per_centre = val == "centre";
    }
    iarg += 2;
  }
  if ((long long) nbin * ntriples > MDP_ADF_MAXCOUNTERS)
    error->all(FLERR, head + std::to_string(nbin) + " bins x " + std::to_string(ntriples) + " triples; the device's histogram holds " +
                          std::to_string(MDP_ADF_MAXCOUNTERS) + " counters");
  if (atom->natoms < 1) error->all(FLERR, "Compute adf/mdp: there are no atoms");
  if (!atom->tag_enable) error->all(FLERR, "Compute adf/mdp requires atom IDs");

  global_array(nbin, 1 + 2 * ntriples);
}

ComputeADFMDP::~ComputeADFMDP() {}

void ComputeADFMDP::init()
{
  require_bricks("where the host's atom->x and neighbour list are current: use compute adf (or run the fix with bricks yes)");
  if (!force->pair) error->all(FLERR, "Compute adf/mdp requires a pair style: its cutforce sets the ghost shell the neighbours come from");
  const double cutforce = force->pair->cutforce;
  if (default_shells) rjout[0] = rkout[0] = cutforce;
  for (int m = 0; m < ntriples; m++) {
    const double outer = rjout[m] > rkout[m] ? rjout[m] : rkout[m];
    if (outer > cutforce * (1.0 + 1e-12)) {
      char buf[320];
      snprintf(buf, sizeof buf, "Compute adf/mdp: the outer radius %g of triple %d is beyond the pair style's cutforce %.15g: the brick's ghost shell is "
                                "cutforce + skin wide as of the last reneighbouring, so only neighbours within cutforce are all present",
               outer, m + 1, cutforce);
      error->all(FLERR, buf);
    }
  }
  // membership by tag for the whole system, made whole over the ranks (compute_rdf_mdp.cpp).  Group all: no table.
  member.clear();
  forget(); // a new init() may bring a new group membership: the setup goes up again
  if (igroup > 0) {
    const bigint n = atom->natoms;
    member.assign((size_t) n, 0);
    for (int i = 0; i < atom->nlocal; i++) {
      const bigint t = atom->tag[i];
      if (t < 1 || t > n) error->one(FLERR, "Compute adf/mdp requires consecutive atom IDs 1 .. natoms");
      if (atom->mask[i] & groupbit) member[(size_t) (t - 1)] = 1;
    }
    sum_whole(member.data(), member.size());
  }
}

void ComputeADFMDP::compute_array()
{
  invoked_array = update->ntimestep;
  mdp_ctx *c = run_context();
  if (!sent(c, mdp_adf_info)) {
    if (mdp_adf_setup(c, nbin, ordinate, ntriples, ilo.data(), ihi.data(), jlo.data(), jhi.data(), klo.data(), khi.data(), rjin.data(),
                      rjout.data(), rkin.data(), rkout.data(), (int) member.size(), member.empty() ? nullptr : member.data()) != MDP_OK)
      fail(c);
    record(c, mdp_adf_info);
  }
  const size_t nh = (size_t) nbin * ntriples, nw = nh + (size_t) ntriples;
  std::vector<long long> cnt(nw, 0);
  if (mdp_adf_counts(c, cnt.data(), cnt.data() + nh) != MDP_OK) fail(c); // (a centre over the neighbour cap ends the run here)
  sum_whole(cnt.data(), nw);

  const double lo = ordinate == MDP_ADF_COSINE ? -1.0 : 0.0;
  const double hi = ordinate == MDP_ADF_DEGREE ? 180.0 : (ordinate == MDP_ADF_RADIAN ? M_PI : 1.0);
  const double delta = (hi - lo) / nbin;
  for (int b = 0; b < nbin; b++) array[b][0] = lo + (b + 0.5) * delta;
  for (int m = 0; m < ntriples; m++) {
    const long long *hist = cnt.data() + (size_t) m * nbin;
    double count = 0.0;
    for (int b = 0; b < nbin; b++) count += (double) hist[b];
    const double den = per_centre ? (double) cnt[nh + m] : count;
    double run = 0.0;
    for (int b = 0; b < nbin; b++) {
      run += (double) hist[b];
      array[b][1 + 2 * m] = count > 0.0 ? (double) hist[b] / (count * delta) : 0.0;
      array[b][2 + 2 * m] = den > 0.0 ? run / den : 0.0;
    }
  }
}
