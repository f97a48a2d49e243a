// `plugin load profilemdpplugin.so`: registers compute profile/mdp (compute_profile_mdp.h), binned temperature, density and
// centre-of-mass velocity of runs that fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_profile_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "profile/mdp", "binned temperature, density and flow on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeProfileMDP>);
}
