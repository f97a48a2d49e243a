// `plugin load indentmdpplugin.so`: registers fix indent/mdp (fix_indent_mdp.h), spherical, cylindrical and planar indenters
// on the device for runs integrated by fix nve/mdp.
#include "mdp_register.h"

#include "fix_indent_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "fix", "indent/mdp", "indenters on the device for runs of fix nve/mdp v1.0", mdp_make3<FixIndentMDP>);
}
