"""Compare the device code of md.hip and langevin.hip at two commits, per kernel.

For both commits compile the two files with
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/F.hip -o DIR/F.s 2> DIR/F.remarks
(no GPU needed) and run
    python profiles/langevin_one_path_asm.py PARENT_DIR THIS_DIR > profiles/langevin_one_path/resources.txt

Every kernel without Langevin arguments, and every LANGEVIN = 0 instantiation of nve_advance_kernel, must be the same
instructions once symbol names and labels are normalised: the script lists any that is not and exits 1.  For the kernels
that carry the Langevin force it prints parent / this of the resources; no scratch, no spill and an occupancy not below
the parent's are asserted, the register counts are reported.
"""
import re
import subprocess
import sys

FILES = ("md", "langevin")
KEYS = ("VGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill",
        "Occupancy [waves/SIMD]")
# parent kernel -> this kernel, where the template arguments changed (the slot count NB in front, LANGEVIN 2 -> 4)
RENAMED = {
    "lgv_final_kernel<false>": "lgv_final_kernel<1, false>", "lgv_final_kernel<true>": "lgv_final_kernel<1, true>",
    "lgv_final_baths_kernel": "lgv_final_kernel<4, true>",
    "lgv_zero_kernel<false>": "lgv_zero_kernel<1, false>", "lgv_zero_kernel<true>": "lgv_zero_kernel<1, true>",
    "lgv_zero_baths_kernel": "lgv_zero_kernel<4, true>",
    "lgv_mean_kernel": "lgv_mean_kernel<1>", "lgv_mean_baths_kernel": "lgv_mean_kernel<4>",
    "lgv_tally_kernel": "lgv_tally_kernel<1>", "lgv_tally_baths_kernel": "lgv_tally_kernel<4>",
}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(full):
    """'(anonymous namespace)::k<a, b>(args)' or 'void (anonymous namespace)::k<a, b>(args)' -> 'k<a, b>'"""
    s = re.sub(r"^void ", "", full).replace("(anonymous namespace)::", "")
    depth = 0
    for n, ch in enumerate(s):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:n]
    return s


def kernels(d):
    """short name -> (normalised instruction lines, resources) of every kernel of the two files in directory d"""
    res = {}
    for f in FILES:
        text = open(f"{d}/{f}.s").read()
        syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
        names = {m: short(full) for m, full in demangle(syms).items()}
        usage, cur = {}, None
        for line in open(f"{d}/{f}.remarks"):
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                cur = usage.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
            if m and cur is not None and m.group(1) in KEYS:
                cur[m.group(1)] = int(m.group(2))
        for sym in syms:
            body = text[text.index(f"\n{sym}:") + 1:]
            body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()].split("\n")[1:]
            labels, lines = {}, []
            for ln in body:
                ln = ln.split(";")[0].rstrip()  # (comments carry source lines and block numbers)
                if not ln.strip() or ln.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
                    continue
                ln = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), ln)
                ln = re.sub(r"_Z\w+", lambda m: names.get(m.group(0), m.group(0)), ln)
                lines.append(ln)
            res[names[sym]] = (lines, usage[sym])
    return res


def main():
    parent, this = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad, rows = [], []
    for name, (lines, use) in parent.items():
        m = re.match(r"nve_advance_kernel<(\w+), (\w+), (\w+), (\d), (\w+)>", name)
        new = RENAMED.get(name, name)
        if m and m.group(4) == "2":
            new = name.replace(", 2, ", ", 4, ")
        langevin = name in RENAMED or (m and m.group(4) != "0")
        if new not in this:
            bad.append(f"{name}: no counterpart {new}")
        elif langevin:
            rows.append((name, new, use, this[new][1], len(lines), len(this[new][0])))
        elif lines != this[new][0] or use != this[new][1]:
            bad.append(f"{name}: differs")
    extra = set(this) - {RENAMED.get(n, n).replace(", 2, ", ", 4, ") if n.startswith("nve_advance") else RENAMED.get(n, n) for n in parent}
    bad += [f"{n}: in this build only" for n in sorted(extra)]
    same = len(parent) - len(rows)
    print(f"{same} kernels of md.hip and langevin.hip without a Langevin force (the 24 LANGEVIN = 0 instantiations of")
    print("nve_advance_kernel among them): " + ("identical instructions and resources after normalising names and labels"
                                                  if not bad else "DIFFERENCES:"))
    for b in bad:
        print("  " + b)
    print()
    print("kernels with the Langevin force, parent / this (lines: instructions and labels):")
    print(f"{'kernel (this build)':<52}{'VGPRs':>9}{'SGPRs':>9}{'LDS':>13}{'scratch':>9}{'spill':>7}{'occup.':>8}{'lines':>11}")
    for name, new, a, b, na, nb in sorted(rows, key=lambda r: r[1]):
        pair = lambda k: f"{a[k]}/{b[k]}"
        spill = f"{a['SGPRs Spill'] + a['VGPRs Spill']}/{b['SGPRs Spill'] + b['VGPRs Spill']}"
        print(f"{new:<52}{pair('VGPRs'):>9}{pair('TotalSGPRs'):>9}{pair('LDS Size [bytes/block]'):>13}"
              f"{pair('ScratchSize [bytes/lane]'):>9}{spill:>7}{pair('Occupancy [waves/SIMD]'):>8}{f'{na}/{nb}':>11}")
        if b["ScratchSize [bytes/lane]"] or b["SGPRs Spill"] or b["VGPRs Spill"]:
            bad.append(f"{new}: scratch or spill")
        if b["Occupancy [waves/SIMD]"] < a["Occupancy [waves/SIMD]"]:
            bad.append(f"{new}: occupancy below the parent's")
    if bad:
        print("\nFAILED:\n  " + "\n  ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
