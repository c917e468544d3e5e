"""scale=None vs scale="ruiz" (power-of-two Ruiz equilibration) over the Netlib fixtures: the standard-form files
(tests/golden/netlib) through solve_with_info and the general-form files (tests/golden/general) through
new_interior_sparse(bounds="native"), each with the reference start and with Mehrotra's start.  One line per file and start:
status, iterations, guarded pivots, auto_regularized, objective error against tests/golden/netlib_optima.json, for the scaled
solve also rp_unscaled / rd_unscaled, the passes used, the log2 spreads of the row maxima before -> after (columns after) and the
device milliseconds of ipm_equilibrate (events on the handle's stream).  The standard-form solves use the device start
(init_state_mehrotra), the general-form ones the host recipe (mehrotra_start), as their entry points do by default.  Nothing is promised about the outcome; files that get worse are listed.

    python tools/scaling_report.py [--set standard|general|both] [--max-iter N] [--limit-seconds S] [--out FILE]

--max-iter: the standard-form set only; new_interior_sparse keeps the reference's fixed 999 iterations and gap tolerance 1e-6.
--limit-seconds: the report stops starting new files once that much wall time has passed (the summary says how many it covered)."""
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
from interiorpointmethod_amd import general_form as G              # noqa: E402
from interiorpointmethod_amd import solver as S                    # noqa: E402
from interiorpointmethod_amd.matio import load_npz_problem         # noqa: E402

OPT = json.load(open(os.path.join(ROOT, "tests", "golden", "netlib_optima.json")))


def load_general(path):
    z = np.load(path)

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))
    return dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


def solve_standard(path, start, scale, max_iter):
    A, b, c, cTlb, valid = load_npz_problem(path)
    if not valid:
        return None
    _, _, _, info = S.solve_with_info(A, b, c, tol=1e-8, max_iter=max_iter, y0=1.0, start=start, device_start=True, scale=scale)
    return info["objective"] - cTlb, info


def solve_general(path, start, scale, max_iter):          # (max_iter: not an argument of new_interior_sparse, see above)
    obj, info = G.new_interior_sparse(**load_general(path), tol=1e-8, return_info=True, start=start, bounds="native", scale=scale)
    return obj, info


def cell(name, res):
    if isinstance(res, str):
        return "ERROR %-60s" % res[:60], False, False
    obj, info = res
    o = OPT.get(name)
    err = abs(obj - o) / max(1.0, abs(o)) if (o is not None and np.isfinite(obj)) else float("nan")
    good = info["status"] == 1 and (o is None or err <= 1e-6)
    txt = "%-9s it=%4d piv=%5d reg=%d err=%8.1e" % (info["status_name"], info["iterations"], info["pivots_fixed"], info["auto_regularized"], err)
    if "scale" in info:
        sc = info["scale"]
        txt += " rpu=%8.1e rdu=%8.1e passes=%2d rows %5.1f->%4.1f cols->%4.1f eq=%6.2fms" % (
            info["rp_unscaled"], info["rd_unscaled"], sc["passes"], sc["row_spread_before"], sc["row_spread_after"], sc["col_spread_after"], float("nan") if sc["ms"] is None else sc["ms"])
    return txt, info["status"] == 1, good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="both", choices=("standard", "general", "both"))
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--limit-seconds", type=float, default=1e9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    t_begin = time.perf_counter()
    sets = []
    if args.set in ("standard", "both"):
        sets.append(("standard", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "netlib", "*.npz"))), solve_standard))
    if args.set in ("general", "both"):
        sets.append(("general", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "general", "*.npz"))), solve_general))
    for label, files, fn in sets:
        emit("# %s form, %d files, tol 1e-8, max_iter %d (general form: the reference's 999 and gap 1e-6), bounds=native" % (label, len(files), args.max_iter))
        tot = {(st, sc): [0, 0] for st in ("reference", "mehrotra") for sc in (None, "ruiz")}
        better, worse, max_passes, covered = [], [], 0, 0
        for f in files:
            if time.perf_counter() - t_begin > args.limit_seconds:
                break
            nm = os.path.basename(f)[:-4]
            skipped = False
            for start in ("reference", "mehrotra"):
                cells = {}
                for scale in (None, "ruiz"):
                    try:
                        res = fn(f, start, scale, args.max_iter)
                    except Exception as e:          # a failed solve is a line of the report, not its end
                        res = "%s: %s" % (type(e).__name__, e)
                    if res is None:
                        skipped = True
                        break
                    txt, conv, good = cell(nm, res)
                    cells[scale] = (txt, good)
                    tot[(start, scale)][0] += conv
                    tot[(start, scale)][1] += good
                    if scale and not isinstance(res, str):
                        max_passes = max(max_passes, res[1]["scale"]["passes"])
                if skipped:
                    break
                emit("%-10s %-3s  off: %s" % (nm, start[:3], cells[None][0]))
                emit("%-10s %-3s ruiz: %s" % (nm, start[:3], cells["ruiz"][0]))
                if cells["ruiz"][1] and not cells[None][1]:
                    better.append("%s/%s" % (nm, start[:3]))
                if cells[None][1] and not cells["ruiz"][1]:
                    worse.append("%s/%s" % (nm, start[:3]))
            covered += not skipped
        emit("# %s summary over %d of %d files (converged / converged to the optimum within 1e-6):" % (label, covered, len(files)))
        for (st, sc), (cv, gd) in tot.items():
            emit("#   start=%-9s scale=%-4s %3d / %3d" % (st, sc, cv, gd))
        emit("#   largest number of passes that changed a factor: %d" % max_passes)
        emit("#   reach the optimum only WITH scaling: %s" % (" ".join(better) or "-"))
        emit("#   reach the optimum only WITHOUT scaling: %s" % (" ".join(worse) or "-"))


if __name__ == "__main__":
    main()
