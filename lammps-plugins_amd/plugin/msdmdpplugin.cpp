// `plugin load msdmdpplugin.so`: registers compute msd/mdp (compute_msd_mdp.h), the mean-squared displacement of runs that
// fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_msd_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "msd/mdp", "mean-squared displacement on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeMSDMDP>);
}
