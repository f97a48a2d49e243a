// `plugin load rdfmdpplugin.so`: registers compute rdf/mdp (compute_rdf_mdp.h), g(r) and coordination numbers of runs that
// fix nve/mdp keeps on the device in bricks mode.
#include "mdp_register.h"

#include "compute_rdf_mdp.h"

using namespace LAMMPS_NS;

extern "C" void lammpsplugin_init(void *lmp, void *handle, void *regfunc)
{
  mdp_register(lmp, handle, regfunc, "compute", "rdf/mdp", "g(r) and coordination numbers on the device for bricks runs of fix nve/mdp v1.0", mdp_make3<ComputeRDFMDP>);
}
