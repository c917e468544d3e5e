"""What LP free columns (ipm_set_free_lp_columns) cost and deliver on the device:

  1. native free columns against the caller's split x = x+ - x- on the same handle kinds, for the constructed problems of
     workloads.free_lp and for block-angular LPs whose linking columns are free: iterations, device ms per iteration, final errors,
     and max(x+ + x-) of the split (its drift along the pair's null direction);
  2. the iteration count and the guarded-pivot count over rho in {1e-4, 1e-6, 1e-8, 1e-10};
  3. the Tikhonov auto-shift on a handle with the set: a problem with 10 % dependent rows;
  4. with --kernel-db DIR (a rocprofv3 --kernel-trace database of a `--kernel-loop` run): the device time of each new kernel beside
     its LP twin, plain and bounded.

    python tools/free_lp_report.py [--out FILE] [--kernel-db DIR]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python tools/free_lp_report.py --kernel-loop
"""
import argparse
import os
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interiorpointmethod_amd import solver as S  # noqa: E402
from interiorpointmethod_amd import workloads  # noqa: E402
from qp_report import Tee, bench_matrix  # noqa: E402

TOL = 1e-8
# (label, m, n, n_free, seed, bounded, as CSC, factor)
PROBLEMS = [("8x20", 8, 20, 3, 7, False, False, None), ("40x130 bounded", 40, 130, 10, 7, True, False, None),
            ("200x520 CSC, envelope factor", 200, 520, 20, 7, False, True, "dense"), ("200x520 CSC, sparse factor", 200, 520, 20, 7, False, True, "sparse"),
            ("1921x4096 (fused launch)", 1921, 4096, 48, 7, False, False, None)]
STEPS = ["prepare", "stop_test", "scaling", "direction", "mu_aff", "corrector_rhs", "update"]


def split_problem(A, c, u, free):
    """x_Phi = x+ - x-: the columns of Phi appended negated, both halves barrier columns."""
    if sparse.issparse(A):
        A2 = sparse.hstack([A, -A[:, free]], format="csc")
    else:
        A2 = np.hstack([A, -A[:, free]])
    c2 = np.concatenate([c, -c[free]])
    u2 = None if u is None else np.concatenate([u, np.full(len(free), np.inf)])
    return A2, c2, u2


def solve(A, b, c, u, free, rho=None, **kw):
    x, y, s, info = S.solve_with_info(A, b, c, ub=u, tol=TOL, max_iter=200, **dict(kw, **({"free_lp": free, "free_rho": rho} if free is not None else {})))
    return x.ravel(), info


def compare(say, label, A, b, c, u, free, x_star=None, obj_star=None, **kw):
    n = A.shape[1]
    xn, a = solve(A, b, c, u, free, **kw)
    A2, c2, u2 = split_problem(A, c, u, free)
    x2, s_ = solve(A2, b, c2, u2, None, **kw)
    xs = x2[:n].copy()
    xs[free] -= x2[n:]
    drift = float(np.max(x2[free] + x2[n:]))

    def err(x, info):
        if x_star is not None:
            return "x_err %.2e" % (np.linalg.norm(x - x_star) / np.linalg.norm(x_star))
        return "obj %.10e" % info["objective"]
    for tag, x, info in (("native", xn, a), ("split", xs, s_)):
        ms = info["solve_ms"] / max(1, info["iterations"])
        say("  %-34s %-6s status %d it %3d  %.4f ms/it  rp %.1e rd %.1e gap %.1e  %s%s%s"
            % (label, tag, info["status"], info["iterations"], ms, info["rp"], info["rd"], info["gap"], err(x, info),
               "" if obj_star is None else "  obj_err %.1e" % (abs(info["objective"] - obj_star) / abs(obj_star)),
               "  max(x+ + x-) %.3e" % drift if tag == "split" else "  fixed pivots %d" % info["pivots_fixed"]))


def rho_sweep(say, label, A, b, c, u, free, **kw):
    for rho in (1e-4, 1e-6, 1e-8, 1e-10):
        x, info = solve(A, b, c, u, free, rho=rho, **kw)
        say("  %-34s rho %.0e  status %d it %3d  fixed pivots %d  auto-shift %d" % (label, rho, info["status"], info["iterations"], info["pivots_fixed"], info["auto_regularized"]))


def kernel_loop(steps):
    for bounded in (False, True):
        A, b, c, u = bench_matrix(4096, 8192, bounded)
        free = np.arange(1, 8192, 128, dtype=np.int32)            # 64 columns outside the bounded (even) ones
        with S.IpmSolver(A, b, c, ub=u) as sv:
            for fr in (None, free):
                sv.set_free_lp(fr)
                sv.init_state(0.0)
                sv.iterate(steps)


def kernel_table(say, path):
    import glob
    import re
    import sqlite3
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
            hit = re.search(r"([a-z_]+_kernel)", name)
            if hit:
                rows[hit.group(1)] = (cnt, avg, mn, mx)
        say("device microseconds per launch at 4096 x 8192 (64 blocks of 256 threads; 64 free columns), LP twin | free_lp kernel:")
        for base in STEPS:
            for mid in ("", "_bounded"):
                lp, fl = "%s%s_kernel" % (base, mid), "%s%s_free_lp_kernel" % (base, mid)
                if lp in rows and fl in rows:
                    say("  %-30s n=%4d avg %7.2f min %7.2f max %7.2f | %-38s n=%4d avg %7.2f min %7.2f max %7.2f" % ((lp,) + rows[lp] + (fl,) + rows[fl]))
                else:
                    say("  %s / %s: not in the trace" % (lp, fl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--kernel-db", default=None)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if args.kernel_loop:
        kernel_loop(args.steps)
        return
    say = Tee(args.out)
    say("LP free columns (ipm_set_free_lp_columns): native against the split x = x+ - x-, tol = %.0e, default rho = 1e-8, reference start" % TOL)
    say()
    say("1. constructed optima (workloads.free_lp) and block-angular LPs with free linking columns:")
    for label, m, n, nf, seed, bounded, as_sparse, factor in PROBLEMS:
        A, b, c, free, u, xs, ys, ss = workloads.free_lp(m, n, nf, seed, bounded=bounded)
        kw = {} if factor is None else {"factor": factor}
        compare(say, label, sparse.csc_matrix(A) if as_sparse else A, b, c, u, free, x_star=xs, obj_star=float(c @ xs), **kw)
    blocks = []
    for m, block, k in ((400, 50, 8), (1200, 100, 16)):
        A, b, c, link = workloads.block_angular_lp(m, block, k, seed=1)
        blocks.append(("block-angular %dx%d, %d free links" % (m, A.shape[1], k), A, b.ravel(), c.ravel(), link.astype(np.int32)))
    for (label, A, b, c, link), kw in zip(blocks, ({"factor": "sparse"}, {})):          # (the larger one's A A^T is too dense for the sparse factor)
        compare(say, label + (", sparse factor" if kw else ", envelope factor"), A, b, c, None, link, **kw)
    say()
    say("2. iterations and guarded pivots over rho:")
    for label, m, n, nf, seed, bounded, as_sparse, factor in PROBLEMS[:4]:
        A, b, c, free, u, xs, ys, ss = workloads.free_lp(m, n, nf, seed, bounded=bounded)
        rho_sweep(say, label, sparse.csc_matrix(A) if as_sparse else A, b, c, u, free, **({} if factor is None else {"factor": factor}))
    A, b, c, free, u, xs, ys, ss = workloads.free_lp(60, 100, 59, 7)
    rho_sweep(say, "60x100 with 59 free columns", A, b, c, u, free)
    label, A, b, c, link = blocks[0]
    rho_sweep(say, label, A, b, c, None, link, factor="sparse")
    say()
    say("3. the Tikhonov auto-shift (more than 5 % guarded pivots at the first factorization): 44 x 130, rows 40 .. 43 copies of rows 0 .. 3")
    A, b, c, free, u, xs, ys, ss = workloads.free_lp(40, 130, 10, 7)
    A4, b4 = np.vstack([A, A[:4]]), np.concatenate([b, b[:4]])
    for rho in (1e-4, 1e-8):
        x, info = solve(A4, b4, c, None, free, rho=rho)
        say("  rho %.0e  status %d it %3d  auto-shift %d  fixed pivots %d  x_err %.2e  rp %.1e rd %.1e"
            % (rho, info["status"], info["iterations"], info["auto_regularized"], info["pivots_fixed"], np.linalg.norm(x - xs) / np.linalg.norm(xs), info["rp"], info["rd"]))
    for rho in (1e-4, 1e-8):          # what the rule would switch on, asked for by hand: the shift is 1e-14 x maxdiag, and maxdiag carries 1 / rho
        x, info = solve(A4, b4, c, None, free, rho=rho, regularize=1e-14)
        say("  rho %.0e with regularize=1e-14: status %d it %3d  fixed pivots %d  x_err %.2e  rp %.1e rd %.1e"
            % (rho, info["status"], info["iterations"], info["pivots_fixed"], np.linalg.norm(x - xs) / np.linalg.norm(xs), info["rp"], info["rd"]))
    x, info = solve(A4, b4, c, None, free, auto_regularize=False)
    say("  rho 1e-08 with auto_regularize=False: status %d it %3d  fixed pivots %d  x_err %.2e" % (info["status"], info["iterations"], info["pivots_fixed"], np.linalg.norm(x - xs) / np.linalg.norm(xs)))
    if args.kernel_db:
        say()
        say("4. the new kernels beside their LP twins (rocprofv3 --kernel-trace of `free_lp_report.py --kernel-loop`):")
        kernel_table(say, args.kernel_db)


if __name__ == "__main__":
    main()
