"""Record tests/golden/variant_bits_parent.json: the bits a build of the PARENT of the class-variant tables computes for every cell of
tests/variant_bits_cases.py (one solve per problem class and launch path).  Needs an MI355X.

    python tools/record_variant_bits.py --root CHECKOUT_OF_THE_PARENT --commit ITS_ID [--out FILE]

CHECKOUT_OF_THE_PARENT is a tree of that commit with its library built (python __graft_entry__.py there); the package is imported
from it, the cells from this tree.  Run once, against the parent, never against a commit that has the tables: the fixture is what
tests/test_gpu_variant_bits.py holds them to.  A cell that runs a solve to its end must reach status 1; if one does not, change
SEED in the cells module -- no cell is left out."""
import argparse
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiler_line():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    return next(ln.strip() for ln in ver.splitlines() if "clang version" in ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "variant_bits_parent.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(args.root))
    import interiorpointmethod_amd as ipm
    import variant_bits_cases as V
    assert os.path.abspath(ipm.__file__).startswith(os.path.abspath(args.root)), ipm.__file__
    got = V.cells(ipm)
    for k, v in sorted(got.items()):
        print("%-24s it=%3d status=%d %s" % (k, v["iterations"], v["status"], v["sha256"][:16]), flush=True)
    bad = [k for k in V.solved_cells(got) if got[k]["status"] != 1]
    if bad:
        sys.exit("cells that did not reach status 1 (change SEED, drop none): %s" % bad)
    with open(args.out, "w") as f:
        json.dump(dict(commit=args.commit, compiler=compiler_line(), seed=V.SEED, cells=got), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cells" % (args.out, len(got)))


if __name__ == "__main__":
    main()
