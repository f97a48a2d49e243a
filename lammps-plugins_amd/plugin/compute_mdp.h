/* -*- c++ -*- -----------------------------------------------------------------------------------
   ComputeMDP: what the /mdp computes share.  They read a run that fix nve/mdp (or fix nvt/mdp, built on it) keeps on the
   device in bricks mode, through the context the run's steps go through (Fix::extract("mdp_steps_ctx")).  Not a style:
   compiled into each compute's plugin file, and it reaches the fix through Fix::extract alone.

     constructor      the two group refusals (unknown, empty) and the head of the derived class' own messages
     gbit()           the group's bit for the library, 0 for group all
     require_bricks   from init(): the one integrator is there, exposes its context and runs in bricks mode
     run_context      from an evaluation: the context of the run under way
     fail             the library's last error, on this rank
     sent / record / forget
                      a context holds one measurement of a kind, and mdp_*_info names it by a serial: the setup goes up
                      once per context, and again when another compute's took its place
     global_array     the storage behind Compute::array
     peratom_columns / read_peratom
                      a per-atom compute: its flags, the storage behind vector_atom / array_atom for atom->nmax atoms, and
                      the hand-over of a read that returns the brick's owned atoms' tags with their values.  On an output
                      step mdp_brick_to_host has just put the brick's owned atoms into the host's arrays in the brick's order,
                      so the tags a read returns are atom->tag[0 .. nlocal) in order; read_peratom checks that.  At the setup
                      of a run (the thermo of step 0) the host still holds its own order: the rows then go to the host's atoms
                      by ID, and an ID the host does not own, or owns twice, fails with a message -- it never hands out
                      misattributed values
     sum_whole        whole numbers summed exactly over the ranks (mdp_whole_sum.h), in place
-------------------------------------------------------------------------------------------------- */
#ifndef MDP_COMPUTE_MDP_H
#define MDP_COMPUTE_MDP_H

#include "compute.h"

#include "mdp_whole_sum.h"
#include "mdpair_hip.h"

#include <string>
#include <vector>

namespace LAMMPS_NS {

class ComputeMDP : public Compute {
 protected:
  // name: "msd/mdp"; empty_tail: what an empty group leaves out, "there is no atom to measure"
  ComputeMDP(class LAMMPS *, int, char **, const char *name, const char *empty_tail);

  const std::string name, head;    // head = "Illegal compute <name> command: "
  typedef int (*info_fn)(mdp_ctx *, long long *);

  int gbit() const { return igroup > 0 ? groupbit : 0; }
  class Fix *integrator() const;
  void require_bricks(const char *hint) const;    // hint: behind "runs in the host-linked mode, "
  mdp_ctx *run_context() const;
  void fail(mdp_ctx *c) const;
  bool sent(mdp_ctx *c, info_fn info);            // our setup is still the one c holds
  void record(mdp_ctx *c, info_fn info);          // ... behind a setup
  void forget() { sent_to = nullptr; }
  void global_array(long long nrows, int ncols);
  typedef int (*peratom_fn)(mdp_ctx *, int *, double *);
  void peratom_columns(int ncols);                // 1: a per-atom vector, more: a per-atom array
  void read_peratom(mdp_ctx *c, peratom_fn read); // read(c, tags, values[nlocal][ncols]) into vector_atom / array_atom

  // v[k] = its sum over the ranks; every |sum| < 2^62.  In pieces: a megabyte of transient buffers whatever n
  template <typename T> void sum_whole(T *v, const size_t n)
  {
    const size_t piece = n < 65536 ? n : 65536;
    std::vector<double> mine(2 * piece), all(2 * piece);
    for (size_t at = 0; at < n; at += piece) {
      const size_t len = n - at < piece ? n - at : piece;
      for (size_t k = 0; k < len; k++) mdp_whole_split((long long) v[at + k], mine[k], mine[len + k]);
      MPI_Allreduce(mine.data(), all.data(), (int) (2 * len), MPI_DOUBLE, MPI_SUM, world);
      for (size_t k = 0; k < len; k++) v[at + k] = (T) mdp_whole_join(all[k], all[len + k]);
    }
  }

 private:
  mdp_ctx *sent_to;    // the context that holds our setup, and which of its measurements is ours
  long long sent_serial;
  std::vector<double> values;
  std::vector<double *> rows;
  int peratom_ncols = 0;
  std::vector<int> peratom_tags;
};

}    // namespace LAMMPS_NS

#endif
