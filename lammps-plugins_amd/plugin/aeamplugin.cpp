// Loader of the MI355X-native `aeam` pair style.  Exports the one C symbol LAMMPS' `plugin load`
// looks up (same contract as lammps/lammps-plugins USER-AEAM/aeamplugin.cpp:14-28), and registers with it the
// time-integration fix that keeps x, v and f on the device for this style (fix_nve_mdp.h).
#include "mdp_register.h"

#include "fix_nve_mdp.h"
#include "pair_aeam.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "pair", "aeam", "angular-EAM pair style, MI355X (gfx950) HIP kernels v1.0", mdp_make1<PairAEAM>);
  mdp_register(lmp, handle, regfunc, "fix", "nve/mdp", "NVE integration on the device for the MI355X pair styles of this plugin v1.0", mdp_make3<FixNVEMDP>);
}
