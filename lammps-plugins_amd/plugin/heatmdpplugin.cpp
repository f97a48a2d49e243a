// `plugin load heatmdpplugin.so`: registers fix heat/mdp (fix_heat_mdp.h), constant-flux heat sources on the device for
// runs integrated by fix nve/mdp.
#include "mdp_register.h"

#include "fix_heat_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "fix", "heat/mdp", "constant-flux heat sources on the device for runs of fix nve/mdp v1.0", mdp_make3<FixHeatMDP>);
}
