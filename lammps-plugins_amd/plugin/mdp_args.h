/* -*- c++ -*- -----------------------------------------------------------------------------------
   Argument parsing of the fixes and the command: a number, a whole number, yes / no.  The callers pass the head of their
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

}    // namespace LAMMPS_NS

#endif
