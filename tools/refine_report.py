"""What iterative refinement of the normal-equations solves buys and costs on the device: status, iterations, the
final primal residual in the caller's units (api.unscaled_residuals), the device milliseconds of the solve (HIP events,
ipm_stats.solve_ms) and the refinement tallies for k = 0, 1, 2 rounds per solve, with both starts, on

  * the Netlib standard-form fixtures (tests/golden/netlib): tol 1e-8, at most --cap-standard iterations (default 300, the cap of
    tools/netlib_report.py --set standard);
  * the Netlib general-form fixtures (tests/golden/general) with native bounds (general_form.native_form): tol 1e-8, e3 = 1e-6, at
    most 999 iterations (what new_interior_sparse runs).

    python tools/refine_report.py [--no-standard] [--no-general] [--round-cost 4096x8192] [--cap-standard N] [--out FILE] [NAME ...]

One handle per (file, start), re-started for every k.  start = reference: x = s = 1, y = 1 (the library's own 5 % rule may switch the
1e-14 shift on: column "shift"); start = mehrotra: ipm_init_state_mehrotra (not refined) with the 5 % rule of handle.mehrotra_started.
A file on the fused small path (one workgroup holds the whole loop; the library refuses k > 0 there) is listed as n/a.  The files
that run with the automatic shift are listed again on their own.  --round-cost MxN: the cost of one refinement round beside one
centrality-corrector round on the dense bench LP, from the phase timers (ipm_set_profiling(2): both are part of "other")."""
import argparse
import glob
import os
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd import api  # noqa: E402
from interiorpointmethod_amd import general_form as G  # noqa: E402
from interiorpointmethod_amd import solver as S  # noqa: E402
from interiorpointmethod_amd.handle import mehrotra_started  # noqa: E402
from interiorpointmethod_amd.matio import load_npz_problem  # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
KS = (0, 1, 2)
STARTS = ("reference", "mehrotra")
PROFILE_STEPS = 8


class Tee:
    def __init__(self, path):
        self.fh = open(path, "w") if path else None

    def __call__(self, line=""):
        print(line, flush=True)
        if self.fh:
            self.fh.write(line + "\n")
            self.fh.flush()


def load_general(path):
    z = np.load(path)

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    F = G.native_form(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                      bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])
    return F.A, F.b, F.c, F.u


def load_standard(path):
    A, b, c, _, _ = load_npz_problem(path)
    return sparse.csc_matrix(A, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel(), None


def run_file(A, b, c, u, start, stop):
    """-> None (small path) or [(stats, refine info, rp_unscaled) for k in KS]."""
    make = lambda **extra: S.IpmSolver(A, b, c, ub=u, **extra)          # noqa: E731
    sv = mehrotra_started(make) if start == "mehrotra" else make()
    with sv:
        if sv.schedule()["fused_small"]:
            return None
        cells = []
        for k in KS:
            sv.set_refine(k)
            if start == "mehrotra":
                sv.init_state_mehrotra()
            else:
                sv.init_state(1.0)
            st = sv.solve(**stop)
            cells.append((st, sv.refine_info(), api.unscaled_residuals(sv)[0]))
        return cells


def run_set(out, title, files, loader, names, stop):
    out("== %s" % title)
    out("%-9s %-9s %6s | %s" % ("file", "start", "shift", "   ".join("k=%d: status   it  rp_unscaled  solve ms  applied/half/rev" % k for k in KS)))
    conv = {(s, k): 0 for s in STARTS for k in KS}
    its = {(s, k): 0 for s in STARTS for k in KS}
    ms = {(s, k): 0.0 for s in STARTS for k in KS}
    gained, lost, shifted, both = [], [], [], 0
    for f in files:
        name = os.path.basename(f)[:-4]
        if names and name not in names:
            continue
        try:
            A, b, c, u = loader(f)
        except Exception as e:
            out("%-9s ERROR loading: %s: %s" % (name, type(e).__name__, e))
            continue
        for start in STARTS:
            try:
                cells = run_file(A, b, c, u, start, stop)
            except Exception as e:           # a failure is a finding of the report, not the end of it
                out("%-9s %-9s ERROR %s: %s" % (name, start, type(e).__name__, e))
                continue
            if cells is None:
                out("%-9s %-9s n/a (fused small path: one workgroup holds the whole loop)" % (name, start))
                continue
            shift = any(st["auto_regularized"] for st, _, _ in cells)
            line = "   ".join("%-9s %4d  %11.3e %9.2f  %4d/%d/%d" % (S.STATUS_NAMES.get(st["status"], "?"), st["iterations"], rp, st["solve_ms"],
                                                                    ri.applied, ri.half_rule, ri.reverts) for st, ri, rp in cells)
            out("%-9s %-9s %6s | %s" % (name, start, "auto" if shift else "-", line))
            if shift:
                shifted.append("%-9s %-9s | %s" % (name, start, line))
            ok = [st["status"] == 1 for st, _, _ in cells]
            for k, good in zip(KS, ok):
                conv[(start, k)] += good
            if all(ok):
                both += 1
                for k, (st, _, _) in zip(KS, cells):
                    its[(start, k)] += st["iterations"]
                    ms[(start, k)] += st["solve_ms"]
            for k, good in zip(KS[1:], ok[1:]):
                if good and not ok[0]:
                    gained.append("%s/%s/k=%d" % (name, start, k))
                if ok[0] and not good:
                    lost.append("%s/%s/k=%d" % (name, start, k))
    out()
    for start in STARTS:
        out("  start %-9s converged: " % start + "   ".join("k=%d: %3d" % (k, conv[(start, k)]) for k in KS))
        out("  start %-9s over the runs that converged for every k: " % start +
            "   ".join("k=%d: %6d it %10.2f ms" % (k, its[(start, k)], ms[(start, k)]) for k in KS))
    out("  moved INTO the converged column by refinement: %s" % (", ".join(gained) if gained else "none"))
    out("  moved OUT of the converged column by refinement: %s" % (", ".join(lost) if lost else "none"))
    out("  runs with the automatic 1e-14 shift:")
    for line in shifted or ["    none"]:
        out("    " + line)
    out()


def round_cost(out, m, n):
    A, b, c = synthetic_lp(m, n)
    with S.IpmSolver(A, b, c) as sv:
        sv.set_profiling(2)
        ph = {}
        for key in ("plain", "refine", "mcc") * 2:                  # (twice: the first pass warms the profiled path up)
            sv.set_refine(1 if key == "refine" else 0)
            sv.set_correctors(1 if key == "mcc" else 0)
            sv.init_state(0.0)
            sv.iterate(PROFILE_STEPS)
            ph[key] = (sv.phase_ms(), sv.refine_info(), sv.corrector_info())
        p0 = ph["plain"][0]["other"]
        pr, ri, _ = ph["refine"]
        pm, _, ci = ph["mcc"]
        rounds_r = max(ri.applied + ri.half_rule + ri.reverts, 1)
        out("== one round at %dx%d (profiling level 2, %d iterations from x = s = 1; 'other' ms per iteration)" % (m, n, PROFILE_STEPS))
        out("   plain %.4f; refine=1 %.4f with %d rounds that did work => %.4f ms per refinement round" %
            (p0, pr["other"], rounds_r, (pr["other"] - p0) * PROFILE_STEPS / rounds_r))
        out("   correctors=1 %.4f with %d rounds that did work => %.4f ms per centrality-corrector round" %
            (pm["other"], ci["rounds"], (pm["other"] - p0) * PROFILE_STEPS / max(ci["rounds"], 1)))
        out("   form %.3f factor %.3f trisolve %.3f ms per iteration" % (ph["plain"][0]["form"], ph["plain"][0]["factor"], ph["plain"][0]["trisolve"]))
        out()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*")
    ap.add_argument("--no-standard", action="store_true")
    ap.add_argument("--no-general", action="store_true")
    ap.add_argument("--round-cost", default=None)
    ap.add_argument("--cap-standard", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = Tee(a.out)
    out("# tools/refine_report.py: iterative refinement of the normal-equations solves, k rounds per solve (DESIGN.md 4-I), one MI355X")
    if a.round_cost:
        round_cost(out, *[int(v) for v in a.round_cost.split("x")])
    if not a.no_standard:
        run_set(out, "Netlib standard form (tests/golden/netlib), tol 1e-8, cap %d" % a.cap_standard,
                sorted(glob.glob(os.path.join(GOLD, "netlib", "*.npz"))), load_standard, set(a.names),
                dict(tol=1e-8, max_iter=a.cap_standard))
    if not a.no_general:
        run_set(out, "Netlib general form, native bounds (tests/golden/general), tol 1e-8, e3 1e-6, cap 999",
                sorted(glob.glob(os.path.join(GOLD, "general", "*.npz"))), load_general, set(a.names),
                dict(tol=1e-8, tol_gap=1e-6, max_iter=999))


if __name__ == "__main__":
    main()
