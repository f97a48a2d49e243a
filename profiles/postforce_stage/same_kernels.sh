#!/bin/bash
# The kernels of indent, spring, heat and md at the parent commit and at this one: the compiler's resource report, one
# line per kernel of the project (its name, 8 hex digits of the sha1 of its mangled name, which tells the template instances apart, then
# SGPRs, VGPRs, AGPRs, scratch bytes per lane, waves per SIMD, LDS bytes per block), and the hash of the disassembly of each
# gfx950 code object with the addresses removed.
# usage: profiles/postforce_stage/same_kernels.sh <checkout of the parent commit>     (no GPU needed)
# writes resources_{parent,this}.txt and disasm_{parent,this}.sha256 next to this file; exit status 1 if they differ
set -eu -o pipefail
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); PARENT=$(cd "$1" && pwd)
ROCM=${ROCM:-/opt/rocm}; T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
for side in parent this; do
  tree=$ROOT; [ $side = parent ] && tree=$PARENT
  mkdir "$T/$side"; : > "$HERE/resources_$side.txt"; : > "$HERE/disasm_$side.sha256"
  for f in indent spring heat md; do
    # (the flags of lammps-plugins_amd/Makefile)
    "$ROCM/bin/hipcc" -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast -munsafe-fp-atomics -Wall -Wno-unused-function \
      -I"$tree/include" -I"$tree/lammps-plugins_amd/csrc" -Rpass-analysis=kernel-resource-usage --save-temps=obj \
      -c "$tree/lammps-plugins_amd/csrc/$f.hip" -o "$T/$side/$f.o" 2> "$T/$side/$f.remarks"
    python3 - "$f" "$T/$side/$f.remarks" >> "$HERE/resources_$side.txt" <<'EOF'
import hashlib, re, sys
want = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
        ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))
name, got, lib = None, {}, []
def flush():
    if name and "rocprim" in name:      # (the library's sort kernels: one line for all of them)
        lib.append(name + " " + " ".join(got[a] for a, b in want))
    elif name:
        m = re.search(r"\d+([a-z]\w*?_kernel)", name)
        short = m.group(1) if m else name
        print(f"{sys.argv[1]}: {short} {hashlib.sha1(name.encode()).hexdigest()[:8]} " + " ".join(f"{b} {got[a]}" for a, b in want))
for line in open(sys.argv[2]):
    m = re.match(r"remark: \S+: +(.*?): (\S+) \[-Rpass", line)
    if not m:
        continue
    if m.group(1) == "Function Name":
        flush()
        name, got = m.group(2), {}
    else:
        got[m.group(1)] = m.group(2)
flush()
if lib:
    print(f"{sys.argv[1]}: {len(lib)} rocprim kernels, sha1 of their names and figures {hashlib.sha1(chr(10).join(sorted(lib)).encode()).hexdigest()}")
EOF
    "$ROCM/llvm/bin/llvm-objdump" -d "$T/$side/$f-hip-amdgcn-amd-amdhsa-gfx950.out" | sed 's/ *\/\/ [0-9A-F]*:.*$//' | grep -v 'file format' \
      > "$T/$side/$f.s"
    echo "$(sha256sum < "$T/$side/$f.s" | cut -d' ' -f1)  $f ($(grep -c '^[0-9a-f]* <' "$T/$side/$f.s") symbols, $(wc -l < "$T/$side/$f.s") lines)" >> "$HERE/disasm_$side.sha256"
  done
done
rc=0
cmp "$HERE/resources_parent.txt" "$HERE/resources_this.txt" || rc=1
cmp "$HERE/disasm_parent.sha256" "$HERE/disasm_this.sha256" || rc=1
for f in indent spring heat md; do diff "$T/parent/$f.s" "$T/this/$f.s" > "$T/$f.diff" || { rc=1; head -40 "$T/$f.diff"; }; done
[ $rc = 0 ] && echo "same kernels: resource reports and disassembly are equal for indent, spring, heat and md"
exit $rc
