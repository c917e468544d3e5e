"""Compare the per-kernel resource figures of two builds: the remarks of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Rpass-analysis=kernel-resource-usage ... csrc/ipm_api.hip  2> LOG
on a parent commit and on this one (a compile: no GPU is needed).

    python tools/resource_compare.py PARENT.log THIS.log [--header TEXT] [--no-scratch REGEX] > profiles/NAME.txt

One line per kernel, named by its demangled signature (c++filt): VGPRs, AGPRs, SGPRs, scratch bytes/lane, LDS bytes/block, occupancy
waves/SIMD, VGPR spills, SGPR spills.  `same` / `DIFF` for every kernel the parent has, then the kernels only this build has.
Exit status 1 when a figure of a parent kernel differs, and, with --no-scratch REGEX, when a kernel of THIS build whose demangled name
matches REGEX has private scratch or a VGPR spill (e.g. --no-scratch '(small_qp\w*_detect|small_lp_batch\w*quad_detect)' for the detecting quadratic
variants of the one-workgroup kernel, whose zero figure rests on keeping loop-invariant addresses out of registers: a compiler that
hoists them again shows up here)."""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return out


def demangle(names):
    """c++filt where the machine has it (binutils); the mangled names otherwise."""
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    return dict(zip(names, r.stdout.split("\n")))


def row(tag, name, fig):
    return "%-6s %-115.115s %s" % (tag, name, " ".join("%6s" % fig.get(f, "?") for f in FIELDS))


def main(argv):
    header = argv[argv.index("--header") + 1] if "--header" in argv else ""
    parent, this = parse(argv[1]), parse(argv[2])
    dm = demangle(sorted(set(parent) | set(this)))
    diff = [k for k in parent if k not in this or this[k] != parent[k]]
    for ln in header.split("\n"):
        if ln:
            print("# " + ln)
    print("# Columns: VGPRs, AGPRs, SGPRs, scratch bytes/lane, LDS bytes/block, occupancy waves/SIMD, VGPR spills, SGPR spills.")
    print("# kernels of the parent: %d; of this commit: %d; parent kernels whose figures differ: %d" % (len(parent), len(this), len(diff)))
    print("#\n# every kernel the parent has (its figures on both commits):")
    for k in sorted(parent, key=lambda k: dm[k]):
        if k in diff:
            print(row("DIFF", dm[k], parent[k]) + "   parent")
            print(row("DIFF", dm[k], this.get(k, {})) + "   this")
        else:
            print(row("same", dm[k], this[k]))
    print("#\n# kernels only this commit has:")
    for k in sorted(set(this) - set(parent), key=lambda k: dm[k]):
        print(row("new", dm[k], this[k]))
    bad = []
    if "--no-scratch" in argv:
        pat = re.compile(argv[argv.index("--no-scratch") + 1])
        held = [k for k in this if pat.search(dm[k])]
        bad = [k for k in held if this[k].get("ScratchSize [bytes/lane]") != "0" or this[k].get("VGPRs Spill") != "0"]
        print("#\n# --no-scratch %r: %d kernels held to 0 bytes of scratch and 0 VGPR spills, %d of them miss it%s"
              % (pat.pattern, len(held), len(bad), "".join("\n#   " + dm[k] for k in bad)))
        if not held:
            bad = ["(no kernel matches)"]
    return 1 if diff or bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
