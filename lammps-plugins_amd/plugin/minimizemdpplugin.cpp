// `plugin load minimizemdpplugin.so`: registers the command style minimize/mdp (command_minimize_mdp.h), the device FIRE
// minimiser for the two pair styles.
#include "mdp_register.h"

#include "command_minimize_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "command", "minimize/mdp", "FIRE minimiser on the device for the rebomos and aeam pair styles v1.0", mdp_make1<MinimizeMDP>);
}
