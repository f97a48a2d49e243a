// `plugin load gforcemdpplugin.so`: registers fix setforce/mdp, fix addforce/mdp and fix aveforce/mdp (fix_gforce_mdp.h),
// prescribed forces on groups on the device for runs integrated by fix nve/mdp.
#include "mdp_register.h"

#include "fix_gforce_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "fix", "setforce/mdp", "fix setforce on the device for runs of fix nve/mdp v1.0", mdp_make3<FixSetForceMDP>);
  mdp_register(lmp, handle, regfunc, "fix", "addforce/mdp", "fix addforce on the device for runs of fix nve/mdp v1.0", mdp_make3<FixAddForceMDP>);
  mdp_register(lmp, handle, regfunc, "fix", "aveforce/mdp", "fix aveforce on the device for runs of fix nve/mdp v1.0", mdp_make3<FixAveForceMDP>);
}
