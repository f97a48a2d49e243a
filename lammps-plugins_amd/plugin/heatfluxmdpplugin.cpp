// `plugin load heatfluxmdpplugin.so`: registers compute heatflux/mdp (compute_heatflux_mdp.h), the heat current of
// runs that fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_heatflux_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "heatflux/mdp", "the heat current from per-atom tallies on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeHeatFluxMDP>);
}
