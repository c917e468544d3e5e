"""Folded against native upper bounds over the general-form fixtures that have finite upper bounds (tests/golden/general):
for each file and each form, the normal-matrix order m, its 128-row blocks, the factor path, the Cholesky flops of one
factorization by the host model (solver.path_flops), iterations and status, the objective error against the Netlib
optimum, the device milliseconds of the solve (HIP events, ipm_stats.solve_ms) and the wall seconds of the whole call.
Same start, tol and e3 for both forms (new_interior_sparse: tol = 1e-8, e3 = 1e-6, at most 999 iterations).

    python tools/bounds_report.py [--start mehrotra|reference] [--repeat R] [--json OUT] [NAME ...]

--repeat R solves each (file, form) R times and reports the median device ms and wall seconds (the first solve of a
file also pays the one-off symbolic analysis of its form on the host)."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd import general_form as G  # noqa: E402
from interiorpointmethod_amd import solver as S  # noqa: E402

GEN = os.path.join(ROOT, "tests", "golden", "general")


def load(path):
    z = np.load(path)

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return z, dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                   bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


def model(A):
    path, fl, _ = S.path_flops(A)
    return path, fl


def run(args, form, start, repeat):
    recs = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        obj, info = G.new_interior_sparse(**args, tol=1e-8, bounds=form, start=start, return_info=True)
        recs.append((time.perf_counter() - t0, info["solve_ms"], obj, info))
    wall = float(np.median([r[0] for r in recs]))
    ms = float(np.median([r[1] for r in recs]))
    return obj, recs[-1][3], ms, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*")
    ap.add_argument("--start", default="mehrotra")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    hdr = "%-9s %-6s %6s %4s %-6s %9s %5s %-9s %9s %9s %8s" % ("file", "form", "m", "blk", "factor", "GF/chol", "it", "status",
                                                            "obj err", "dev ms", "wall s")
    print(hdr, flush=True)
    for f in sorted(glob.glob(os.path.join(GEN, "*.npz"))):
        name = os.path.basename(f)[:-4]
        if a.names and name not in a.names:
            continue
        z, args = load(f)
        if not np.isfinite(z["ub"]).any():
            continue
        opt = float(z["netlib_optimum"])
        for form in ("fold", "native"):
            if form == "fold":
                A = G.standard_form(**args)[0]
            else:
                A = G.native_form(**args).A
            m = A.shape[0]
            path, fl = model(sparse.csc_matrix(A))
            try:
                obj, info, ms, wall = run(args, form, a.start, a.repeat)
            except Exception as e:           # a failure is a finding of the report, not the end of it
                print("%-9s %-6s ERROR %s: %s" % (name, form, type(e).__name__, e), flush=True)
                rows.append(dict(file=name, form=form, m=m, error="%s: %s" % (type(e).__name__, e)))
                continue
            err = abs(obj - opt) / max(1.0, abs(opt))
            r = dict(file=name, form=form, m=m, blocks=(m + 127) // 128, factor=info["factor_path"], chol_gflop=fl / 1e9,
                     model_path=path, iterations=info["iterations"], status=info["status_name"], obj=obj, netlib=opt,
                     rel_err=err, device_ms=ms, wall_s=wall, bounded=info.get("bounded", 0),
                     fixed_removed=info.get("fixed_removed", 0))
            rows.append(r)
            print("%-9s %-6s %6d %4d %-6s %9.3f %5d %-9s %9.1e %9.2f %8.3f" % (name, form, m, r["blocks"], r["factor"], r["chol_gflop"],
                                                                              r["iterations"], r["status"], err, ms, wall), flush=True)
    # summary: native / folded device time per file
    print("\n%-9s %10s %10s %8s" % ("file", "fold ms", "native ms", "ratio"))
    by = {}
    for r in rows:
        if "device_ms" in r:
            by.setdefault(r["file"], {})[r["form"]] = r
    for name, d in sorted(by.items()):
        if "fold" in d and "native" in d:
            print("%-9s %10.2f %10.2f %8.2f" % (name, d["fold"]["device_ms"], d["native"]["device_ms"],
                                                d["native"]["device_ms"] / max(d["fold"]["device_ms"], 1e-9)))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(start=a.start, repeat=a.repeat, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
