/* ------------------------------------------------------------------------------------------------
   MI355X-native REBO Mo-S pair style: LAMMPS-facing adapter (host C++).

   Mirrors the host-visible behaviour of lammps/lammps-plugins USER-REBOMOS/pair_rebomos.cpp:
   constructor flags (:57-72), settings (:144-147), coeff (:153-203), init_style (:209-238),
   init_one (:244-274), compute (:102-111) and the error messages of each.  The force/energy
   arithmetic itself (REBO_neigh, FREBO, bondorder, FLJ) runs in hand-written HIP kernels behind the
   C-ABI of include/mdpair_hip.h.

   Differences a host can observe, by design:
     * owner-computes: compute() adds complete forces to OWNED atoms and nothing to ghosts, so the
       host's reverse_comm of f carries zeros for this style;
     * the global virial is tallied explicitly on the device (no_virial_fdotr = 1), because
       x.f over ghosts is only valid for the scatter formulation;
     * per-atom virial (compute stress/atom) is complete on owned atoms, nothing on ghosts.
-------------------------------------------------------------------------------------------------- */
#include "pair_rebomos.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "memory.h"
#include "neigh_list.h"
#include "neighbor.h"
#include "output.h"
#include "update.h"
#include "utils.h"

#include <cstring>
#include <string>

using namespace LAMMPS_NS;

PairREBOMoS::PairREBOMoS(LAMMPS *lmp) : PairMDP(lmp, "rebomos", 1)
{
  // pair_rebomos.cpp:59-64
  single_enable = 0;
  restartinfo = 0;
  one_coeff = 1;
  ghostneigh = 1;
  manybody_flag = 1;
  centroidstressflag = CENTROID_NOTAVAIL;
  // the device tallies the pair virial itself (see header comment)
  no_virial_fdotr = 1;

  overflow_is_neigh_one = true;    // pair_rebomos.cpp:350
  params_read = false;
  cut3rebo = 0.0;
  device_bytes = 0.0;
  memset(&params, 0, sizeof params);
}

void PairREBOMoS::coeff(int narg, char **arg)
{
  coeff_args(narg, arg);

  // atom type -> element: Mo (or legacy M) = 0, S = 1, NULL = -1   (pair_rebomos.cpp:168-179)
  map[0] = -1;
  for (int i = 3; i < narg; i++) {
    int el;
    if (strcmp(arg[i], "NULL") == 0)
      el = -1;
    else if (strcmp(arg[i], "Mo") == 0 || strcmp(arg[i], "M") == 0)
      el = 0;
    else if (strcmp(arg[i], "S") == 0)
      el = 1;
    else
      error->all(FLERR, "Incorrect args for pair coefficients");
    map[i - 2] = el;
  }

  // potential file: 61 scalars + mixing rules, shared front end in libmdpair_hip.so
  char why[512] = "";
  const std::string path = utils::get_potential_file_path(arg[2]);
  if (mdp_rebomos_read_file(path.empty() ? arg[2] : path.c_str(), &params, why, (int) sizeof why) != MDP_OK)
    error->one(FLERR, why[0] ? why : "reading rebomos potential file failed");
  params_read = true;
  if (dev && mdp_rebomos_set_params(dev, &params) != MDP_OK) fail_one(MDP_EINVAL, "parameter upload");

  coeff_setflags();
}

void PairREBOMoS::init_style()
{
  if (atom->tag_enable == 0) error->all(FLERR, "Pair style REBOMoS requires atom IDs");
  if (force->newton_pair == 0) error->all(FLERR, "Pair style REBOMoS requires newton pair on");
  // atom types mapped to NULL (pair hybrid) are invisible to the device lists: map[] = -1 goes down as is

  // full neighbor list including neighbors of ghosts (pair_rebomos.cpp:218)
  neighbor->add_request(this, NeighConst::REQ_FULL | NeighConst::REQ_GHOST);

  if (open_device() && params_read && mdp_rebomos_set_params(dev, &params) != MDP_OK) fail_one(MDP_EINVAL, "parameter upload");
  nall_uploaded = -1;
  // MDP_REBOMOS_HOST_LIST=1: the lists are subsets of the rows LAMMPS built (exclusions and special bonds act as in the
  // reference) instead of being built from the positions -- see mdp_rebomos_host_list
  const char *ehl = getenv("MDP_REBOMOS_HOST_LIST");
  host_list = ehl && atoi(ehl) != 0;
  if (mdp_rebomos_host_list(dev, host_list ? 1 : 0) != MDP_OK) fail_one(MDP_EINVAL, "list mode");
}

double PairREBOMoS::init_one(int i, int j)
{
  if (setflag[i][j] == 0) error->all(FLERR, "All pair coeffs are not set");
  const int ii = map[i], jj = map[j];
  // list cutoff = 3 REBO distances of the largest element; ghost-list cutoff = REBO cutoff
  // (pair_rebomos.cpp:257-261)
  cut3rebo = 3.0 * params.rcmax[0][0];
  cutghost[i][j] = cutghost[j][i] = params.rcmax[ii][jj];
  return cut3rebo;
}

void PairREBOMoS::compute(int eflag, int vflag)
{
  ev_init(eflag, vflag);
  if (bricks) {
    compute_bricks();
    return;
  }

  if (linked() && host_list)
    error->all(FLERR, "Pair style rebomos (MI355X): fix nve/mdp keeps the atoms on the device and cannot be combined with MDP_REBOMOS_HOST_LIST=1");
  // the box of this step: on one periodic rank the library gives the images their positions itself, as
  // Comm::forward_comm does (owner + whole box vectors), and takes the owned atoms' positions only
  // (lists from the host's rows: the rows index the host's own ghosts, which then come up with the positions)
  const bool linked = upload_host({comm->nprocs == 1 && !host_list ? domain->h : nullptr, map, host_list, list->gnum, true,
                                   mdp_rebomos_check_host_list, cut3rebo + neighbor->skin});

  const int nlocal = atom->nlocal;
  const int ef = (eflag_global ? MDP_EFLAG_GLOBAL : 0) | (eflag_atom ? MDP_EFLAG_ATOM : 0);
  const int vf = (vflag_global ? MDP_VFLAG_GLOBAL : 0) | (vflag_atom ? MDP_VFLAG_ATOM : 0);
  // the forces' only reader is on the device too -- unless the host tallies or writes something this step
  const bool f_stays = linked && !ef && !vf && update->ntimestep != output->next;
  const int rc = mdp_rebomos_compute_host(dev, ef, vf, (nlocal && !f_stays) ? atom->f[0] : nullptr, &eng_vdwl, virial, eatom,
                                          (vflag_atom && vatom) ? vatom[0] : nullptr);
  if (rc != MDP_OK) fail_one(rc, "compute");
}

void *PairREBOMoS::extract(const char *str, int &dim)
{
  // for a context of the fix's (or minimize/mdp's) own: the style's parameters
  dim = 0;
  if (strcmp(str, "mdp_rebomos_params") == 0) return params_read ? (void *) &params : nullptr;
  if (strcmp(str, "mdp_map") == 0) return (void *) map;
  return PairMDP::extract(str, dim);
}

double PairREBOMoS::memory_usage()
{
  // the reference reports the REBO lists it holds (pair_rebomos.cpp:1113-1124); here they live on the device:
  // candidate / tile lists, slot forces, staging of x and f -- plus the pinned host staging of one x and one f array
  device_bytes = dev ? mdp_device_bytes(dev) : 0.0;
  double bytes = device_bytes;
  bytes += (double) (atom->nlocal + atom->nghost) * (3 * sizeof(double) + sizeof(int));
  return bytes;
}
