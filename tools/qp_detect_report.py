"""What the infeasibility tests of a quadratic handle (IPM_FLAG_DETECT_QUADRATIC, detect_qp=True) cost on one MI355X:

  1. device milliseconds per iteration (HIP events: ipm_stats.solve_ms of ipm_solve over the iterations it ran) of a FLAGGED against
     an UNFLAGGED quadratic handle on the same data: dense 4096 x 8192 (the fused launch, the residual stream), a sparse-factor
     problem (block_angular_lp(4000, 50, 0) with a diagonal: 0.27 ms per iteration), and a 36 x 146 factor-model QP on the one-workgroup path.  ipm_solve, not ipm_iterate:
     the stop test of ipm_iterate skips the tests.  The tolerances are set so that nothing converges and nothing fires within the
     steps taken; median and range over --reps runs;
  2. wall seconds of the 64-member return-target sweep of tests/qp_infeas_cases.py (three infeasible members) through
     solve_small_factor_qp_batch (the three run to the cap) and solve_small_factor_qp_batch_detect (they end in status 5).

    python tools/qp_detect_report.py [--out FILE] [--steps K] [--reps R] [--unflagged-only]

The sweep of part 2 is the one the GPU test uses: this tool imports tests/qp_infeas_cases.py (it puts tests/ on sys.path), so it
needs the tests directory of the checkout next to it.
--unflagged-only: the unflagged legs alone (what a tree without the flag can run: the baseline of "no regression")."""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ms_per_iteration(make, steps, reps):
    out = []
    with make() as sv:
        sv.init_state(1.0)
        sv.solve(tol=1e-300, max_iter=2)                  # warm-up
        for _ in range(reps):
            sv.init_state(1.0)
            st = sv.solve(tol=1e-300, max_iter=steps)
            assert st["iterations"] == steps and st["status"] == 2, "the leg must run its %d steps: status %d after %d" % (steps, st["status"], st["iterations"])
            out.append(st["solve_ms"] / steps)
        path = "one-workgroup" if sv.schedule()["fused_small"] else "fused launch" if sv.schedule()["fused_factor"] else "factor=%s" % sv.factor
    return float(np.median(out)), min(out), max(out), path


def legs(say, label, args_, kw, steps, reps, unflagged_only):
    from interiorpointmethod_amd import IpmSolver
    rows = {}
    for leg in ("unflagged",) if unflagged_only else ("unflagged", "flagged", "unflagged again"):
        extra = dict(detect_qp=True, infeasibility_tol=(1e-300, 1e-300)) if leg == "flagged" else {}
        rows[leg] = ms_per_iteration(lambda: IpmSolver(*args_, **dict(kw, **extra)), steps, reps)
        say("  %-44s %-16s median %.4f ms/iteration (min %.4f, max %.4f; %d x %d steps; %s)" % ((label, leg) + rows[leg][:3] + (reps, steps, rows[leg][3])))
    if not unflagged_only:
        off = 0.5 * (rows["unflagged"][0] + rows["unflagged again"][0])
        say("  %-44s flagged - unflagged = %+.4f ms (%+.2f %%); the two unflagged legs differ by %.2f %%"
            % (label, rows["flagged"][0] - off, 100 * (rows["flagged"][0] - off) / off, 100 * abs(rows["unflagged"][0] - rows["unflagged again"][0]) / off))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--unflagged-only", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import interiorpointmethod_amd as ipm
    from interiorpointmethod_amd import factor_qp_form, workloads
    say("# tools/qp_detect_report.py%s: the infeasibility tests of a quadratic handle on one MI355X (DESIGN.md 4-V)" % (" --unflagged-only" if a.unflagged_only else ""))
    say("1. device ms per iteration of ipm_solve, unflagged against flagged quadratic handle (same data, fresh handle per leg):")
    A, b, c, g, u, xs, ys = workloads.separable_qp(4096, 8192, 0)
    legs(say, "separable QP, dense 4096 x 8192", (A, b, c), dict(quad=g), a.steps, a.reps, a.unflagged_only)
    A, b, c, _ = workloads.block_angular_lp(4000, 50, 0, seed=1)
    gs = np.random.default_rng(5).uniform(0.1, 2.0, A.shape[1])
    legs(say, "block_angular_lp(4000, 50, 0), sparse factor", (sparse.csc_matrix(A), b.ravel(), c.ravel()), dict(quad=gs, factor="sparse"), a.steps, a.reps, a.unflagged_only)
    A, b, c, g, F, u, xs, ys = workloads.factor_qp(30, 140, 6, 7)
    A_, b_, c_, g_, u_, free = factor_qp_form(sparse.csc_matrix(A), b, c, g, F, u)
    legs(say, "factor-model QP 36 x 146, one-workgroup path", (A_, b_, c_), dict(quad=g_, free=free, free_small=True), a.steps, a.reps, a.unflagged_only)
    say()
    say("2. wall seconds of the 64-member return-target sweep (three infeasible members), one ipm_solve_small_batch call each, max_iter 5000:")
    import qp_infeas_cases as QC
    problems = QC.return_target_sweep()
    fns = [("solve_small_factor_qp_batch", ipm.solve_small_factor_qp_batch)]
    if not a.unflagged_only:
        fns.append(("solve_small_factor_qp_batch_detect", ipm.solve_small_factor_qp_batch_detect))
    for name, fn in fns:
        fn(problems[:2], max_iter=50)                       # warm-up
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn(problems)
            ts.append(time.perf_counter() - t0)
        st = [o[3]["status"] for o in out]
        it = [o[3]["iterations"] for o in out]
        say("  %-36s median %.3f s (min %.3f, max %.3f; %d runs); statuses of the last three members %s after %s iterations; the other 61: status %s, at most %d iterations"
            % (name, float(np.median(ts)), min(ts), max(ts), a.reps, st[-3:], it[-3:], sorted(set(st[:-3])), max(it[:-3])))


if __name__ == "__main__":
    main()
