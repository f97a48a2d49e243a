// `plugin load cnamdpplugin.so`: registers compute cna/atom/mdp (compute_cna_atom_mdp.h), the per-atom common neighbour
// analysis of runs that fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_cna_atom_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "cna/atom/mdp", "per-atom common neighbour analysis on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeCnaAtomMDP>);
}
