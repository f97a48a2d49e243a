/* -*- c++ -*- -----------------------------------------------------------------------------------
   Argument parsing of the fixes, the computes and the command: a number, a whole number, yes / no, a range of atom types.  The callers pass the head of their
   own messages ("Illegal fix nvt/mdp command: ", "minimize/mdp: ").
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_ARGS_H
#define MDP_ARGS_H

#include "error.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

namespace LAMMPS_NS {

// the whole of s is a number (finite: and neither inf nor nan)
inline bool mdp_number(const char *s, double &v, bool finite = false)
{
  char *end = nullptr;
  v = strtod(s, &end);
  return end != s && *end == '\0' && (!finite || std::isfinite(v));
}

inline bool mdp_whole(const char *s, long long &v)
{
  char *end = nullptr;
  v = strtoll(s, &end, 10);
  return end != s && *end == '\0';
}

// ... or "<head>bad <what> value <s>"
inline double mdp_number(Error *error, const std::string &head, const std::string &what, const char *s, bool finite = false)
{
  double v = 0.0;
  if (!mdp_number(s, v, finite)) error->all(FLERR, head + "bad " + what + " value " + s);
  return v;
}

// ... or "<head><key> takes yes or no", with ", not <s>" behind it where the caller names the value
inline bool mdp_yesno(Error *error, const std::string &head, const std::string &key, const char *s, bool name_value)
{
  if (strcmp(s, "yes") != 0 && strcmp(s, "no") != 0)
    error->all(FLERR, head + key + " takes yes or no" + (name_value ? std::string(", not ") + s : std::string()));
  return s[0] == 'y';
}

// a LAMMPS type argument N, *, N*, *M or N*M over 1 .. ntypes (utils::bounds)
inline bool mdp_type_bounds(const std::string &s, const int ntypes, int &lo, int &hi)
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

}    // namespace LAMMPS_NS

#endif
