// `plugin load springmdpplugin.so`: registers fix spring/mdp (fix_spring_mdp.h), tether springs on the centre of mass of a
// group on the device for runs integrated by fix nve/mdp.
#include "mdp_register.h"

#include "fix_spring_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "fix", "spring/mdp", "tether springs on the device for runs of fix nve/mdp v1.0", mdp_make3<FixSpringMDP>);
}
