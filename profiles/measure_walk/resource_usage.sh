#!/bin/sh
# The compiler's resource report of the four neighbour-measurement kernels (no GPU needed): run from the repository root,
#   sh profiles/measure_walk/resource_usage.sh > profiles/measure_walk/this_resource_usage.txt
# and the same in a checkout of the parent commit for parent_resource_usage.txt.  The command line is the Makefile's own for
# csrc/<name>.o (its HIPFLAGS), asked of make, with the device-only remark options in front of -c and no object kept.
cd "$(dirname "$0")/../../lammps-plugins_amd" || exit 1
for f in adf coord centro rdf; do
  cmd=$(make -n -B csrc/$f.o | grep -- " -c csrc/$f.hip") || exit 1
  eval "$(echo "$cmd" | sed "s# -c csrc/$f.hip -o csrc/$f.o# --cuda-device-only -Rpass-analysis=kernel-resource-usage -c csrc/$f.hip -o /dev/null#")" 2>&1 | sed "s#^csrc/##"
done
