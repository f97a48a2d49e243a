#!/usr/bin/env python3
"""Per-kernel resources of a built libmdpair_hip.so, read from the gfx950 code objects inside it (no GPU involved):

    python profiles/kernel_resources.py lammps-plugins_amd/libmdpair_hip.so > new.txt

prints one line per kernel, sorted by name -- VGPRs, AGPRs, SGPRs, scratch and LDS bytes as the code object's metadata
states them and a hash of the kernel's machine code -- so that `diff` of two builds' outputs shows whether a change
that is not meant to touch device code has left it alone.  Needs llvm-readelf and llvm-objdump of the ROCm LLVM."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    blob = open(path, "rb").read()
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        q = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + 1)


def kernels(obj_bytes):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj_bytes)
        f.flush()
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", f.name], check=True, capture_output=True, text=True).stdout
        syms = subprocess.run([LLVM + "/llvm-readelf", "-sW", f.name], check=True, capture_output=True, text=True).stdout
        secs = subprocess.run([LLVM + "/llvm-readelf", "-SW", f.name], check=True, capture_output=True, text=True).stdout
    m = re.search(r"^\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", secs, re.M)
    text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
    code = {}
    for line in syms.splitlines():
        p = line.split()
        if len(p) == 8 and p[3] == "FUNC":
            a, size = int(p[1], 16), int(p[2])
            code[p[7]] = hashlib.sha256(obj_bytes[text_off + a - text_addr:text_off + a - text_addr + size]).hexdigest()[:16]
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = ".agpr_count:" + block
        g = lambda k: re.search(r"\.%s:\s*'?([^'\n]+)'?" % k, block).group(1).strip()
        name = g("name")
        out[name] = (int(g("vgpr_count")), int(g("agpr_count")), int(g("sgpr_count")), int(g("private_segment_fixed_size")),
                     int(g("group_segment_fixed_size")), code.get(name, "?"))
    return out


def main():
    allk = {}
    for obj in code_objects(sys.argv[1]):
        for name, v in kernels(obj).items():
            allk.setdefault(name, set()).add(v) # a template kernel of a header is emitted once per file that uses it
    print("# kernel vgpr agpr sgpr scratch lds code-sha256[:16]")
    for name in sorted(allk):
        for v in sorted(allk[name]):
            print(name, *v)
    print("# %d kernels" % len(allk))


if __name__ == "__main__":
    main()
