/* -*- c++ -*- -----------------------------------------------------------------------------------
   A 64-bit integer as two whole-number doubles, for an exact sum through MPI_SUM of MPI_DOUBLE (the one reduction the
   mini-host's MPI subset has): q = hi 2^31 + lo with 0 <= lo < 2^31.  Summed over the ranks both halves stay whole numbers
   below 2^53, and the join gives the integer sum.  No shift of a signed value on either side.  Nothing but <cmath>, so
   that a stand-alone program can include it (tests/native/asan_check.cpp); ComputeMDP::sum_whole is the reduction.
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_WHOLE_SUM_H
#define MDP_WHOLE_SUM_H

#include <cmath>

namespace LAMMPS_NS {

inline void mdp_whole_split(const long long q, double &hi, double &lo)
{
  const long long low = q & 2147483647ll;
  hi = (double) ((q - low) / 2147483648ll); // (exact: q - low is a multiple of 2^31)
  lo = (double) low;
}

inline long long mdp_whole_join(const double hi, const double lo) { return llrint(hi) * 2147483648ll + llrint(lo); }

}    // namespace LAMMPS_NS

#endif
