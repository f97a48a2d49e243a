/* ------------------------------------------------------------------------------------------------
   MI355X-native angular-EAM pair style: LAMMPS-facing adapter (host C++).

   Mirrors the host-visible behaviour of lammps/lammps-plugins USER-AEAM/pair_aeam.cpp:
   constructor flags (:36-59), settings (:513-517), coeff (:523-595), init_style (:601-609),
   init_one (:615-621), the comm callbacks (:946-990) and compute (:110-479) with their error
   messages.  Density, embedding and force passes run in HIP kernels behind include/mdpair_hip.h.

   compute() = density half on the device -> this style's own forward_comm of fp (as the reference
   does at :307, but here the exchange is REQUIRED: ghosts' fp feed the gather formulation) -> force
   half.  Forces on ghosts are produced only by angular (three-body) centres and are folded by the
   host's reverse_comm of f, as for the reference.
-------------------------------------------------------------------------------------------------- */
#include "pair_aeam.h"

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

PairAEAM::PairAEAM(LAMMPS *lmp) : PairMDP(lmp, "aeam", 2)
{
  // pair_aeam.cpp:38-58
  restartinfo = 0;
  manybody_flag = 1;
  unit_convert_flag = utils::get_supported_conversions(utils::ENERGY);
  comm_forward = 1;
  comm_reverse = 1;
  one_coeff = 1;
  no_virial_fdotr = 1;    // explicit pair virial from the device (gather formulation)

  nmax = 0;
  rho = fp = nullptr;
  cutforcesq = cutmax = 0.0;
  potfile = nullptr;
  tables_built = false;
  nelements = 0;
  cut_el = nullptr;
  device_lists = false;
  memset(&tables, 0, sizeof tables);
}

PairAEAM::~PairAEAM()
{
  memory->destroy(rho);
  memory->destroy(fp);
  if (potfile) mdp_aeam_file_free(potfile);
}

void PairAEAM::coeff(int narg, char **arg)
{
  coeff_args(narg, arg);

  // potential file (pair_aeam.cpp:536-551)
  if (potfile) {
    mdp_aeam_file_free(potfile);
    potfile = nullptr;
  }
  tables_built = false;
  char why[512] = "";
  const std::string path = utils::get_potential_file_path(arg[2]);
  if (mdp_aeam_file_read(path.empty() ? arg[2] : path.c_str(), &potfile, why, (int) sizeof why) != MDP_OK)
    error->one(FLERR, why[0] ? why : "Cannot open AEAM potential file");
  char names[MAXEL * 16 + 16] = "";
  int nnon = 0, nang = 0;
  mdp_aeam_file_info(potfile, &nelements, &nnon, &nang, element_mass, MAXEL, names, (int) sizeof names);
  {
    int k = 0;
    char *save = nullptr;
    for (char *tok = strtok_r(names, " ", &save); tok && k < MAXEL; tok = strtok_r(nullptr, " ", &save), k++) {
      strncpy(elements[k], tok, 15);
      elements[k][15] = 0;
    }
  }

  // map atom types to elements (pair_aeam.cpp:555-566) ...
  for (int i = 3; i < narg; i++) {
    if (strcmp(arg[i], "NULL") == 0) {
      map[i - 2] = -1;
      continue;
    }
    int j;
    for (j = 0; j < nelements; j++)
      if (strcmp(arg[i], elements[j]) == 0) break;
    if (j < nelements)
      map[i - 2] = j;
    else
      error->all(FLERR, "No matching element in AEAM potential file");
  }
  // ... and insist on the file's element order (pair_aeam.cpp:568-572)
  for (int i = 3; i < narg; i++)
    if (i - 3 >= nelements || strcmp(arg[i], elements[i - 3]) != 0)
      error->all(FLERR, "no matching atom order of input file and potential file");

  coeff_setflags(element_mass);
}

void PairAEAM::init_style()
{
  if (force->newton_pair == 0) error->all(FLERR, "Pair style aeam requires newton pair on");

  // file2array + array2spline (pair_aeam.cpp:605-606), then the tables go to the device
  if (!potfile) error->all(FLERR, "All pair coeffs are not set");
  if (mdp_aeam_file_build(potfile, atom->ntypes, map, &tables) != MDP_OK)
    error->all(FLERR, "Pair style aeam (MI355X): building the spline tables failed");
  tables_built = true;
  cut_el = const_cast<double *>(tables.cut);
  open_device();
  if (mdp_aeam_set_tables(dev, &tables) != MDP_OK) fail_one(MDP_EINVAL, "table upload");
  // lists built on the device from the positions (the host's list is only checked); MDP_AEAM_HOST_LIST=1 streams
  // the host's list instead
  const char *ehl = getenv("MDP_AEAM_HOST_LIST");
  device_lists = !(ehl && atoi(ehl) != 0);
  if (mdp_aeam_device_lists(dev, device_lists ? 1 : 0) != MDP_OK) fail_one(MDP_EINVAL, "list mode");

  neighbor->add_request(this, NeighConst::REQ_FULL);
  nall_uploaded = -1;
}

double PairAEAM::init_one(int i, int j)
{
  if (setflag[i][j] == 0) error->all(FLERR, "All pair coeffs are not set");
  // per-type-pair cutoff straight from the file (pair_aeam.cpp:618-620)
  cutmax = tables_built ? tables.cut[(i - 1) * tables.nelements + (j - 1)] : 0.0;
  cutforcesq = cutmax * cutmax;
  return cutmax;
}

void PairAEAM::compute(int eflag, int vflag)
{
  ev_init(eflag, vflag);
  if (bricks) {
    compute_bricks();
    return;
  }

  if (atom->nmax > nmax) {
    memory->destroy(rho);
    memory->destroy(fp);
    nmax = atom->nmax;
    memory->create(rho, nmax, "pair:rho");
    memory->create(fp, nmax, "pair:fp");
  }

  // the box of this step: on one periodic rank the library keeps the images itself (positions, fp, their share of the
  // three-body forces), as Comm::forward_comm / reverse_comm would; the lists as init_style chose
  const bool linked = upload_host({comm->nprocs == 1 ? domain->h : nullptr, nullptr, !device_lists, 0, false,
                                   mdp_aeam_check_host_list, neighbor->skin});
  const int nall = atom->nlocal + atom->nghost;
  const int ef = (eflag_global ? MDP_EFLAG_GLOBAL : 0) | (eflag_atom ? MDP_EFLAG_ATOM : 0);
  const int vf = (vflag_global ? MDP_VFLAG_GLOBAL : 0) | (vflag_atom ? MDP_VFLAG_ATOM : 0);

  // passes 1+2 on the device; fp (owned) comes back for the halo -- unless every ghost is an image the library keeps
  // itself: then rho and fp (private to this class, as in the reference) never leave the device
  const bool local_halo = mdp_host_ghosts_derived(dev) == 1;
  int rc = mdp_aeam_density_host(dev, ef, local_halo ? nullptr : fp, local_halo ? nullptr : rho, &eng_vdwl, eatom);
  if (rc != MDP_OK) fail_one(rc, "density pass");

  // communicate the derivative of the embedding function (pair_aeam.cpp:307)
  if (!local_halo) comm->forward_comm(this);

  // (linked to fix nve/mdp: the forces' only reader is on the device too -- unless the host tallies or writes this step)
  const bool f_stays = linked && local_halo && !ef && !vf && update->ntimestep != output->next;
  rc = mdp_aeam_force_host(dev, ef, vf, local_halo ? nullptr : fp, (nall && !f_stays) ? atom->f[0] : nullptr, &eng_vdwl,
                           virial, eatom, (vflag_atom && vatom) ? vatom[0] : nullptr);
  if (rc != MDP_OK) fail_one(rc, "force pass");
}

void *PairAEAM::extract(const char *str, int &dim)
{
  // for a context of the fix's (or minimize/mdp's) own: the style's tables
  dim = 0;
  if (strcmp(str, "mdp_aeam_tables") == 0) return tables_built ? (void *) &tables : nullptr;
  return PairMDP::extract(str, dim);
}

/* ---- per-pair comm callbacks, same packing as pair_aeam.cpp:946-990 ---------------------------- */

int PairAEAM::pack_forward_comm(int n, int *list, double *buf, int /*pbc_flag*/, int * /*pbc*/)
{
  int m = 0;
  for (int i = 0; i < n; i++) buf[m++] = fp[list[i]];
  return m;
}

void PairAEAM::unpack_forward_comm(int n, int first, double *buf)
{
  int m = 0;
  const int last = first + n;
  for (int i = first; i < last; i++) fp[i] = buf[m++];
}

int PairAEAM::pack_reverse_comm(int n, int first, double *buf)
{
  // the device computes rho for owned atoms from the full list; ghosts carry nothing
  int m = 0;
  const int last = first + n;
  for (int i = first; i < last; i++) buf[m++] = 0.0;
  return m;
}

void PairAEAM::unpack_reverse_comm(int n, int *list, double *buf)
{
  int m = 0;
  for (int i = 0; i < n; i++) rho[list[i]] += buf[m++];
}

double PairAEAM::memory_usage()
{
  double bytes = (double) maxeatom * sizeof(double);
  bytes += (double) maxvatom * 6 * sizeof(double);
  bytes += 2.0 * nmax * sizeof(double);
  if (dev) bytes += mdp_device_bytes(dev); // repacked list, spline tables and work arrays held on the GPU
  return bytes;
}
