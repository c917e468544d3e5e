"""What the separable convex QP (ipm_set_quadratic) costs and delivers on the device:

  1. device milliseconds per iteration (HIP events, ipm_stats.solve_ms of ipm_iterate), LP against QP on the SAME handle and the same
     A -- the dense 4096 x 8192 bench matrix, plain and bounded, and one sparse-factor problem (block_angular_lp) -- the term switched
     with set_quadratic between the legs;
  2. iterations and final errors against the constructed optimum of the workloads.separable_qp problems the tests solve;
  3. with --kernel-db DIR (a rocprofv3 --kernel-trace database of a `--kernel-loop` run): the device time of the four Quad kernels
     beside their LP twins, plain and bounded.

    python tools/qp_report.py [--out FILE] [--steps K] [--reps R] [--kernel-db DIR]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python tools/qp_report.py --kernel-loop

The LP legs use the data of the QP (its c included): ipm_iterate takes its steps without a stop decision, so both legs enqueue the
same number of iterations from the same start whatever they converge to."""
import argparse
import glob
import os
import re
import sqlite3
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd import solver as S  # noqa: E402
from interiorpointmethod_amd import workloads  # noqa: E402

PROBLEMS = [("300x700", 300, 700, 1, False, False, None), ("300x700 bounded, mixed", 300, 700, 2, True, True, None),
            ("200x520 bounded, CSC, envelope factor", 200, 520, 3, True, False, "dense"),
            ("200x520 bounded, CSC, sparse factor", 200, 520, 3, True, False, "sparse"), ("2560x5120", 2560, 5120, 4, False, False, None)]
TWINS = ["prepare", "scaling", "mu_aff", "update"]


class Tee:
    def __init__(self, path):
        self.fh = open(path, "w") if path else None

    def __call__(self, line=""):
        print(line, flush=True)
        if self.fh:
            self.fh.write(line + "\n")
            self.fh.flush()


def diagonal(n, seed=0):
    return np.random.default_rng(seed).uniform(0.1, 2.0, n)


def bench_matrix(m, n, bounded):
    A, b, c = workloads.synthetic_lp(m, n, seed=0)
    u = None
    if bounded:
        u = np.full(n, np.inf)
        u[::2] = 3.0                                  # x0 < 1.5 stays strictly inside
    return A, b.ravel(), c.ravel(), u


def ms_per_iteration(sv, steps, reps):
    sv.init_state(0.0)
    sv.iterate(3)                                     # warm-up
    out = []
    for _ in range(reps):
        sv.init_state(0.0)
        out.append(sv.iterate(steps)["solve_ms"] / steps)
    return float(np.median(out)), min(out), max(out)


def timing_leg(say, label, sv, g, steps, reps):
    rows = {}
    for leg in ("LP", "QP", "LP again"):
        sv.set_quadratic(g if leg == "QP" else None)
        rows[leg] = ms_per_iteration(sv, steps, reps)
        say("  %-44s %-9s median %.4f ms/iteration (min %.4f, max %.4f; %d x %d steps)" % ((label, leg) + rows[leg] + (reps, steps)))
    lp = 0.5 * (rows["LP"][0] + rows["LP again"][0])
    say("  %-44s QP - LP = %+.4f ms (%+.2f %%); the two LP legs differ by %.2f %%"
        % (label, rows["QP"][0] - lp, 100 * (rows["QP"][0] - lp) / lp, 100 * abs(rows["LP"][0] - rows["LP again"][0]) / lp))


def kernel_loop(steps):
    for bounded in (False, True):
        A, b, c, u = bench_matrix(4096, 8192, bounded)
        with S.IpmSolver(A, b, c, ub=u) as sv:
            for g in (None, diagonal(sv.n)):
                sv.set_quadratic(g)
                sv.init_state(0.0)
                sv.iterate(steps)


def kernel_table(say, path):
    dbs = [path] if path.endswith(".db") else glob.glob(os.path.join(path, "**", "*.db"), recursive=True)
    for db in dbs:
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type='table'")]
        kt = [t for t in tabs if "kernel_dispatch" in t][0]
        sym = [t for t in tabs if "kernel_symbol" in t][0]
        q = ("select s.kernel_name, count(*), avg(k.end-k.start)/1e3, min(k.end-k.start)/1e3, max(k.end-k.start)/1e3 "
             "from %s k join %s s on k.kernel_id=s.id group by s.kernel_name" % (kt, sym))
        rows = {}
        for name, cnt, avg, mn, mx in con.execute(q).fetchall():
            hit = re.search(r"([a-z_]+_kernel)", name)              # demangled ipm::NAME(...) or mangled _ZN3ipm<len>NAME...
            if hit:
                rows[hit.group(1)] = (cnt, avg, mn, mx)
        say("device microseconds per launch at 4096 x 8192 (64 blocks of 256 threads), LP twin | Quad kernel:")
        for base in TWINS:
            for mid in ("", "_bounded"):
                lp, qp = "%s%s_kernel" % (base, mid), "%s%s_quad_kernel" % (base, mid)
                if lp in rows and qp in rows:
                    say("  %-24s n=%4d avg %7.2f min %7.2f max %7.2f | %-30s n=%4d avg %7.2f min %7.2f max %7.2f"
                        % ((lp,) + rows[lp] + (qp,) + rows[qp]))
                else:
                    say("  %s / %s: not in the trace" % (lp, qp))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--kernel-db", default=None)
    args = ap.parse_args()
    if args.kernel_loop:
        kernel_loop(args.steps)
        return
    say = Tee(args.out)
    say("# tools/qp_report.py: the separable convex QP on one MI355X (DESIGN.md 4-Q)")
    say("1. device ms per iteration, LP against QP on the same handle (ipm_iterate, HIP events):")
    for bounded in (False, True):
        A, b, c, u = bench_matrix(4096, 8192, bounded)
        with S.IpmSolver(A, b, c, ub=u) as sv:
            timing_leg(say, "dense 4096 x 8192%s" % (", half bounded" if bounded else ""), sv, diagonal(sv.n), args.steps, args.reps)
            say("  (fused formation + factorization launch in use: fused_factor = %d)" % sv.schedule()["fused_factor"])
    A, b, c, _ = workloads.block_angular_lp(4000, 50, 0, seed=1)
    with S.IpmSolver(A, b.ravel(), c.ravel(), factor="sparse") as sv:
        timing_leg(say, "block_angular_lp(4000, 50, 0) %d x %d, factor=%s" % (sv.m, sv.n, sv.factor), sv, diagonal(sv.n), args.steps, args.reps)
    say()
    say("2. whole solves of workloads.separable_qp (reference start, tol 1e-8): status, iterations, errors against the constructed optimum")
    for label, m, n, seed, bounded, mixed, factor in PROBLEMS:
        A, b, c, g, u, xs, ys = workloads.separable_qp(m, n, seed, bounded=bounded, mixed=mixed)
        kw = {} if factor is None else {"factor": factor}
        with S.IpmSolver(sparse.csc_matrix(A) if factor else A, b, c, ub=u, quad=g, **kw) as sv:
            sv.init_state(1.0)
            st = sv.solve(tol=1e-8)
            x, y, s = (v.ravel() for v in sv.get_state())
            obj = float(c @ xs + 0.5 * (g * xs) @ xs)
            say("  %-40s status %d iterations %2d  |x - x*|/|x*| %.2e  |y - y*|/|y*| %.2e  objective error %.2e  rp %.1e rd %.1e gap %.1e  %.2f ms"
                % (label, st["status"], st["iterations"], np.linalg.norm(x - xs) / np.linalg.norm(xs), np.linalg.norm(y - ys) / np.linalg.norm(ys),
                   abs(st["objective"] - obj) / abs(obj), st["rp_norm"] / (1 + st["b_norm"]), st["rd_norm"] / (1 + st["c_norm"]), st["gap"], st["solve_ms"]))
    if args.kernel_db:
        say()
        say("3. the four Quad kernels beside their LP twins (rocprofv3 --kernel-trace of `qp_report.py --kernel-loop`):")
        kernel_table(say, args.kernel_db)


if __name__ == "__main__":
    main()
