"""What Gondzio's centrality correctors buy and cost on the device: iterations, rounds that did work / were
accepted and the device milliseconds of the solve (HIP events, ipm_stats.solve_ms) for K = 0 .. 3 rounds per iteration at
eta = 0.91 (the default) and eta = 0.995, and the cost of one round from the phase timers.

    python tools/correctors_report.py [--sizes 4096x8192,8192x16384] [--no-dense] [--no-netlib] [--repeat R] [--out FILE] [NAME ...]

Dense: the bench LP (workloads.synthetic_lp, start x = s = 1, y = 0) solved to tol 1e-8.  One handle per (size, eta); per K one
warm-up solve, then R timed ones: median and span of solve_ms.  The cost of a round: ipm_set_profiling(2) (the plain path, no
residual stream), iterate(8) from the start with K = 0 and K = 3; the rounds are part of phase 3 ("everything else"), so one round
costs (other_K3 - other_K0) * 8 / rounds that did work.  Printed beside half of phase 2 (the two Mehrotra solves), which is what one
more solve with the factor costs.

Netlib: the general-form fixtures (tests/golden/general) with native bounds (general_form.native_form) from Mehrotra's start on the
device, tol 1e-8, e3 = 1e-6, at most 999 iterations (what new_interior_sparse runs).  One handle per (file, eta), re-started for every
K; median solve_ms of R solves.  A file on the fused small path (one workgroup holds the whole loop; the library refuses K > 0
there) is listed as n/a.  NAME ...: only these files."""
import argparse
import glob
import os
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd import general_form as G  # noqa: E402
from interiorpointmethod_amd import solver as S  # noqa: E402
from interiorpointmethod_amd.handle import mehrotra_started  # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp  # noqa: E402

GEN = os.path.join(ROOT, "tests", "golden", "general")
ETAS = (0.91, 0.995)
KS = (0, 1, 2, 3)
PROFILE_STEPS = 8


class Tee:
    def __init__(self, path):
        self.fh = open(path, "w") if path else None

    def __call__(self, line=""):
        print(line, flush=True)
        if self.fh:
            self.fh.write(line + "\n")
            self.fh.flush()


def load(path):
    z = np.load(path)

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return z, dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                   bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


def timed(sv, start, K, repeat, **stop):
    """-> (stats of the last solve, corrector info, [solve_ms]) of `repeat` solves from start() with K rounds, after one warm-up."""
    sv.set_correctors(K)
    ms = []
    for i in range(repeat + 1):
        start()
        st = sv.solve(**stop)
        if i:
            ms.append(st["solve_ms"])
    return st, sv.corrector_info(), ms


def dense(out, sizes, repeat):
    out("== dense synthetic LP (bench family), start x = s = 1, y = 0, tol 1e-8; solve_ms: median [min .. max] of %d solves" % repeat)
    out("%-13s %-6s %2s %5s %7s %9s %10s   %s" % ("size", "eta", "K", "it", "rounds", "accepted", "solve ms", "[min .. max]"))
    for m, n in sizes:
        A, b, c = synthetic_lp(m, n)
        for eta in ETAS:
            with S.IpmSolver(A, b, c, eta=eta) as sv:
                for K in KS:
                    st, ci, ms = timed(sv, lambda: sv.init_state(0.0), K, repeat, tol=1e-8, max_iter=300)
                    out("%-13s %-6g %2d %5d %7d %9d %10.3f   [%.3f .. %.3f]  %s" % ("%dx%d" % (m, n), eta, K, st["iterations"], ci["rounds"],
                                                                                    ci["accepted"], float(np.median(ms)), min(ms), max(ms),
                                                                                    S.STATUS_NAMES.get(st["status"], "?")))
                if eta == ETAS[0]:
                    sv.set_profiling(2)
                    ph = {}
                    for K in (0, 3, 0, 3):                  # (twice: the first pair warms the profiled path up)
                        sv.set_correctors(K)
                        sv.init_state(0.0)
                        sv.iterate(PROFILE_STEPS)
                        ph[K] = (sv.phase_ms(), sv.corrector_info()["rounds"])
                    sv.set_profiling(0)
                    (p0, _), (p3, r3) = ph[0], ph[3]
                    per_round = (p3["other"] - p0["other"]) * PROFILE_STEPS / max(r3, 1)
                    out("   round cost %dx%d (profiling level 2, first %d iterations): other %.4f -> %.4f ms/iteration with %d rounds "
                        "=> %.4f ms per round; half of the two Mehrotra solves (phase 2 / 2) %.4f ms; form %.3f factor %.3f ms"
                        % (m, n, PROFILE_STEPS, p0["other"], p3["other"], r3, per_round, p0["trisolve"] / 2, p0["form"], p0["factor"]))
        del A
    out()


def netlib(out, names, repeat):
    out("== Netlib general form, native bounds, Mehrotra start on the device, tol 1e-8, e3 1e-6, cap 999; solve_ms: median of %d" % repeat)
    out("%-9s %6s %-6s %-6s | %s" % ("file", "m", "factor", "eta", "   ".join("K=%d: it rounds/acc     ms" % K for K in KS)))
    total = {(eta, K): 0.0 for eta in ETAS for K in KS}
    iters = {(eta, K): 0 for eta in ETAS for K in KS}
    counted = 0
    for f in sorted(glob.glob(os.path.join(GEN, "*.npz"))):
        name = os.path.basename(f)[:-4]
        if names and name not in names:
            continue
        try:
            F = G.native_form(**load(f)[1])
            rows = {}
            for eta in ETAS:
                make = lambda **extra: S.IpmSolver(F.A, F.b, F.c, ub=F.u, eta=eta, **extra)          # noqa: E731
                with mehrotra_started(make) as sv:
                    if sv.schedule()["fused_small"]:
                        rows = None
                        out("%-9s %6d %-6s n/a (fused small path: one workgroup holds the whole loop)" % (name, sv.m, "small"))
                        break
                    cells = []
                    for K in KS:
                        st, ci, ms = timed(sv, sv.init_state_mehrotra, K, repeat, tol=1e-8, tol_gap=1e-6, max_iter=999)
                        cells.append((st, ci, float(np.median(ms))))
                    rows[eta] = (sv.m, sv.factor, cells)
            if rows is None:
                continue
        except Exception as e:           # a failure is a finding of the report, not the end of it
            out("%-9s ERROR %s: %s" % (name, type(e).__name__, e))
            continue
        ok = all(st["status"] == 1 for eta in ETAS for st, _, _ in rows[eta][2])
        for eta in ETAS:
            m, fac, cells = rows[eta]
            out("%-9s %6d %-6s %-6g | %s%s" % (name, m, fac, eta, "   ".join("%4d %4d/%-4d %9.2f" % (st["iterations"], ci["rounds"], ci["accepted"], ms)
                                                                             for st, ci, ms in cells),
                                               "" if all(st["status"] == 1 for st, _, _ in cells) else "   status " + ",".join(
                                                   S.STATUS_NAMES.get(st["status"], "?") for st, _, _ in cells)))
            if ok:
                for K, (st, ci, ms) in zip(KS, cells):
                    total[(eta, K)] += ms
                    iters[(eta, K)] += st["iterations"]
        counted += ok
    out()
    out("totals over the %d files that converged in all eight runs: iterations / solve ms" % counted)
    for eta in ETAS:
        out("  eta %-6g " % eta + "   ".join("K=%d: %6d it %10.2f ms" % (K, iters[(eta, K)], total[(eta, K)]) for K in KS))
    out()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*")
    ap.add_argument("--sizes", default="4096x8192,8192x16384")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--no-netlib", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = Tee(a.out)
    out("# tools/correctors_report.py: centrality correctors, K rounds per iteration (DESIGN.md 4-G), one MI355X")
    if not a.no_dense:
        dense(out, [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s], a.repeat)
    if not a.no_netlib:
        netlib(out, set(a.names), a.repeat)


if __name__ == "__main__":
    main()
