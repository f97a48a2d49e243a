// `plugin load centromdpplugin.so`: registers compute centro/atom/mdp (compute_centro_atom_mdp.h), the per-atom centro-symmetry
// parameter of runs that fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_centro_atom_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "centro/atom/mdp", "per-atom centro-symmetry parameter on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeCentroAtomMDP>);
}
