/* -*- c++ -*- -----------------------------------------------------------------------------------
   MI355X-native angular-EAM pair style: LAMMPS-facing adapter.

   Same class name, style name and virtual surface as the CPU plugin
   (lammps/lammps-plugins USER-AEAM/pair_aeam.h:14-41), including the four per-pair comm callbacks.
   All arithmetic happens in libmdpair_hip.so (include/mdpair_hip.h); what this adapter shares with the rebomos one is
   its base class (pair_mdp.h).
-------------------------------------------------------------------------------------------------- */
#ifdef PAIR_CLASS
// clang-format off
PairStyle(aeam,PairAEAM);
// clang-format on
#else

#ifndef MDP_PAIR_AEAM_H
#define MDP_PAIR_AEAM_H

#include "pair_mdp.h"

namespace LAMMPS_NS {

class PairAEAM : public PairMDP {
 public:
  PairAEAM(class LAMMPS *);
  ~PairAEAM() override;
  void compute(int, int) override;
  void coeff(int, char **) override;
  void init_style() override;
  double init_one(int, int) override;

  int pack_forward_comm(int, int *, double *, int, int *) override;
  void unpack_forward_comm(int, int, double *) override;
  int pack_reverse_comm(int, int, double *) override;
  void unpack_reverse_comm(int, int *, double *) override;
  double memory_usage() override;
  void *extract(const char *, int &) override;

 protected:
  int nmax;                   // allocated size of the per-atom host arrays
  double cutforcesq, cutmax;
  double *rho, *fp;           // host mirrors: rho (owned), fp = Fptmp*F' (owned, then ghosts via forward_comm)

  mdp_aeam_file *potfile;     // parsed AlSi.aeam-style file (owns the table storage)
  mdp_aeam_tables tables;
  bool tables_built;
  int nelements;
  static constexpr int MAXEL = 64; // (a bound on what a file may declare; everything else is sized from the file)
  char elements[MAXEL][16];
  double element_mass[MAXEL];
  double *cut_el;             // [nelements*nelements], points into potfile
  bool device_lists;          // lists built on the device from the positions; the host's list is checked, not read
};

}    // namespace LAMMPS_NS

#endif
#endif
