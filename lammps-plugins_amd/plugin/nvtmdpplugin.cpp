// `plugin load nvtmdpplugin.so`: registers fix nvt/mdp (fix_nvt_mdp.h), the device thermostat for the pair styles of
// rebomosplugin.so and aeamplugin.so.
#include "mdp_register.h"

#include "fix_nvt_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "fix", "nvt/mdp", "Nose-Hoover chain NVT on the device for the MI355X pair styles v1.0", mdp_make3<FixNVTMDP>);
}
