// `plugin load coordmdpplugin.so`: registers compute coord/atom/mdp (compute_coord_atom_mdp.h), per-atom coordination numbers of
// runs that fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_coord_atom_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "coord/atom/mdp", "per-atom coordination numbers on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeCoordAtomMDP>);
}
