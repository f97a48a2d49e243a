// `plugin load adfmdpplugin.so`: registers compute adf/mdp (compute_adf_mdp.h), bond-angle distributions of runs that
// fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_adf_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "adf/mdp", "bond-angle distributions on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeADFMDP>);
}
