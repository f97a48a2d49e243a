// `plugin load langevinmdpplugin.so`: registers fix langevin/mdp (fix_langevin_mdp.h), the device Langevin thermostat
// for runs integrated by fix nve/mdp.
#include "mdp_register.h"

#include "fix_langevin_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "fix", "langevin/mdp", "Langevin thermostat on the device for runs of fix nve/mdp v1.0", mdp_make3<FixLangevinMDP>);
}
