"""What free columns with curvature (ipm_set_free_columns) and the factor-model QP built on them cost and deliver:

  1. device milliseconds per iteration (HIP events, ipm_stats.solve_ms of ipm_iterate) of a quadratic handle with the free set ON,
     CLEARED and ON again, on the SAME handle: the augmented form of a factor-model QP on the dense 4096 x 8192 bench shape with
     k = 64 (the fused launch), plain and bounded, and of a block-angular sparse problem with 16 sector factors (each loads on a
     sixteenth of the columns) on the envelope factor and on the sparse factor;
  2. whole solves of workloads.factor_qp through solve_factor_qp: iterations and errors against the constructed optimum;
  3. device microseconds per launch of each Free kernel beside its Quad or LP twin (rocprofv3 --kernel-trace of the --kernel-loop leg).

    python tools/factor_qp_report.py [--out profiles/factor_qp_report.txt] [--steps K] [--reps R] [--no-trace]

Every GPU step is a child process under a time limit of its own; the report stops at the first step that fails or runs out of time.
ipm_iterate takes its steps without a stop decision, so the legs of part 1 enqueue the same number of iterations from the same start."""
import argparse
import glob
import os
import re
import shutil
import signal
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVES = [("1x64 k=8 bounded", 1, 64, 8, True, None), ("40x130 k=8 bounded", 40, 130, 8, True, None), ("300x700 k=64", 300, 700, 64, False, None),
          ("200x520 k=16, CSC, envelope factor", 200, 520, 16, False, "dense"), ("200x520 k=16, CSC, sparse factor", 200, 520, 16, False, "sparse"),
          ("2560x5120 k=64 (fused launch)", 2560, 5120, 64, False, None)]
# Free kernel -> its twin on the same handle with the set cleared (a Quad kernel where the step has one, else the LP's)
TWINS = [("prepare", "prepare%s_quad_kernel"), ("scaling", "scaling%s_quad_kernel"), ("stop_test", "stop_test%s_kernel"), ("direction", "direction%s_kernel"),
         ("mu_aff", "mu_aff%s_quad_kernel"), ("corrector_rhs", "corrector_rhs%s_kernel"), ("update", "update%s_quad_kernel")]
LIMITS = {"timing": 420, "solves": 240, "trace": 300}          # seconds per GPU step


def dense_problem(bounded):
    from interiorpointmethod_amd import factor_qp_form, workloads
    A, b, c, g, F, u, xs, ys = workloads.factor_qp(4096, 8192, 64, 0, bounded=bounded)
    return factor_qp_form(A, b, c, g, F, u)


def sparse_problem():
    from interiorpointmethod_amd import factor_qp_form, workloads
    A, b, c, _ = workloads.block_angular_lp(2000, 50, 0, seed=1)
    n = A.shape[1]
    rng = np.random.default_rng(5)
    F = np.zeros((n, 16))                             # sector factors: factor f loads on its own sixteenth of the columns, so the rows
    sector = np.arange(n) * 16 // n                   # [F^T -I] stay sparse and A_ A_^T keeps a sparse factor
    F[np.arange(n), sector] = rng.standard_normal(n) / np.sqrt(n / 16.0)
    return factor_qp_form(sparse.csc_matrix(A), b.ravel(), c.ravel(), rng.uniform(0.1, 2.0, n), F)


def ms_per_iteration(sv, steps, reps):
    sv.init_state(1.0)
    sv.iterate(2)                                     # warm-up
    out = []
    for _ in range(reps):
        sv.init_state(1.0)
        out.append(sv.iterate(steps)["solve_ms"] / steps)
    return float(np.median(out)), min(out), max(out)


def timing_leg(label, sv, free, steps, reps):
    rows = {}
    for leg in ("free on", "cleared", "on again"):
        sv.set_free(None if leg == "cleared" else free)
        rows[leg] = ms_per_iteration(sv, steps, reps)
        print("  %-46s %-9s median %.4f ms/iteration (min %.4f, max %.4f; %d x %d steps)" % ((label, leg) + rows[leg] + (reps, steps)), flush=True)
    on = 0.5 * (rows["free on"][0] + rows["on again"][0])
    off = rows["cleared"][0]
    print("  %-46s on - cleared = %+.4f ms (%+.2f %%); the two legs with the set on differ by %.2f %%"
          % (label, on - off, 100 * (on - off) / off, 100 * abs(rows["free on"][0] - rows["on again"][0]) / on), flush=True)


def step_timing(steps, reps):
    from interiorpointmethod_amd import solver as S
    for bounded in (False, True):
        A_, b_, c_, g_, u_, free = dense_problem(bounded)
        with S.IpmSolver(A_, b_, c_, ub=u_, quad=g_, free=free) as sv:
            timing_leg("dense %d x %d (4096 x 8192, k = 64)%s" % (sv.m, sv.n, ", bounded" if bounded else ""), sv, free, steps, reps)
            print("  (fused formation + factorization launch in use: fused_factor = %d)" % sv.schedule()["fused_factor"], flush=True)
    A_, b_, c_, g_, u_, free = sparse_problem()
    for factor in ("dense", "sparse"):
        with S.IpmSolver(A_, b_, c_, quad=g_, free=free, factor=factor) as sv:
            timing_leg("block_angular_lp(2000, 50, 0) + 16 sector factors: %d x %d, factor=%s" % (sv.m, sv.n, sv.factor), sv, free, steps, reps)


def step_solves():
    import interiorpointmethod_amd as ipm
    from interiorpointmethod_amd import workloads
    for label, m, n, k, bounded, factor in SOLVES:
        A, b, c, g, F, u, xs, ys = workloads.factor_qp(m, n, k, 7, bounded=bounded)
        kw = {} if factor is None else {"factor": factor}
        x, y, s, info = ipm.solve_factor_qp(sparse.csc_matrix(A) if factor else A, b, c, F, g=g, ub=u, tol=1e-8, **kw)
        x, y, ts = x.ravel(), y.ravel(), F.T @ xs
        obj = float(c @ xs + 0.5 * (g * xs) @ xs + 0.5 * ts @ ts)
        print("  %-36s status %d iterations %2d  |x - x*|/|x*| %.2e  |y - y*|/|y*| %.2e  |t - F^T x| %.2e  objective error %.2e  rp %.1e rd %.1e gap %.1e  %.2f ms"
              % (label, info["status"], info["iterations"], np.linalg.norm(x - xs) / np.linalg.norm(xs), np.linalg.norm(y - ys) / np.linalg.norm(ys),
                 np.linalg.norm(info["t"] - F.T @ x), abs(info["objective"] - obj) / abs(obj), info["rp"], info["rd"], info["gap"], info["solve_ms"]), flush=True)


def step_kernel_loop(steps):
    from interiorpointmethod_amd import solver as S
    for bounded in (False, True):
        A_, b_, c_, g_, u_, free = dense_problem(bounded)
        with S.IpmSolver(A_, b_, c_, ub=u_, quad=g_, free=free) as sv:
            for fr in (free, None):
                sv.set_free(fr)
                sv.init_state(1.0)
                sv.iterate(steps)


def kernel_table(path):
    dbs = glob.glob(os.path.join(path, "**", "*.db"), recursive=True)
    if not dbs:
        print("  no kernel-trace database was written under %s" % path)
        return
    rows = {}
    con = sqlite3.connect(dbs[0])
    tabs = [r[0] for r in con.execute("select name from sqlite_master where type='table'")]
    kt = [t for t in tabs if "kernel_dispatch" in t][0]
    sym = [t for t in tabs if "kernel_symbol" in t][0]
    q = ("select s.kernel_name, count(*), avg(k.end-k.start)/1e3, min(k.end-k.start)/1e3, max(k.end-k.start)/1e3 "
         "from %s k join %s s on k.kernel_id=s.id group by s.kernel_name" % (kt, sym))
    for name, cnt, avg, mn, mx in con.execute(q).fetchall():
        hit = re.search(r"([a-z_]+_kernel)", name)                  # demangled ipm::NAME(...) or mangled _ZN3ipm<len>NAME...
        if hit:
            rows[hit.group(1)] = (cnt, avg, mn, mx)
    print("device microseconds per launch at 4160 x 8256 (33 blocks of 256 threads; stop_test: one thread), twin | Free kernel:")
    for base, twin in TWINS:
        for mid in ("", "_bounded"):
            a, f = twin % mid, "%s%s_free_kernel" % (base, mid)
            if a in rows and f in rows:
                print("  %-32s n=%4d avg %7.2f min %7.2f max %7.2f | %-34s n=%4d avg %7.2f min %7.2f max %7.2f" % ((a,) + rows[a] + (f,) + rows[f]))
            else:
                print("  %s / %s: not in the trace" % (a, f))


def child(step, args, out, prefix=()):
    """One GPU step in a process of its own, under its time limit; its output goes to the report.  False: the report stops here."""
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps), "--reps", str(args.reps)]
    limit = LIMITS["trace" if prefix else step]
    # a process group of its own: under the profiler the process that holds the GPU is a grandchild, and the limit must end it too
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT, start_new_session=True)
    try:
        stdout, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        out("  step %s ran past its %d s limit; the report stops here" % (step, limit))
        return False
    for line in stdout.splitlines():
        if line.startswith("  "):                     # the step's own lines (the runtime's and the profiler's chatter is not indented)
            out(line)
    if p.returncode != 0:
        for line in stdout.splitlines()[-6:]:
            out("  | " + line)
        out("  step %s ended with exit status %d; the report stops here" % (step, p.returncode))
    return p.returncode == 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_qp_report.txt"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kernel-db", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "timing":
        return step_timing(args.steps, args.reps)
    if args.step == "solves":
        return step_solves()
    if args.step == "kernel-loop":
        return step_kernel_loop(args.steps)
    if args.step == "kernel-table":
        return kernel_table(args.kernel_db)
    fh = open(args.out, "w")

    def out(line=""):
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()
    out("# tools/factor_qp_report.py: free columns with curvature and factor-model QPs on one MI355X (DESIGN.md 4-U)")
    out("1. device ms per iteration of a quadratic handle with the free set on, cleared and on again, same handle (ipm_iterate, HIP events):")
    if not child("timing", args, out):
        return 1
    out()
    out("2. whole solves of workloads.factor_qp (seed 7) through solve_factor_qp (reference start, tol 1e-8) against the constructed optimum:")
    if not child("solves", args, out):
        return 1
    prof = shutil.which("rocprofv3")
    if args.no_trace or not prof:
        out()
        out("3. kernel trace not taken (%s)" % ("--no-trace" if args.no_trace else "rocprofv3 not found"))
        return 0
    out()
    out("3. the Free kernels beside their twins (rocprofv3 --kernel-trace of the --kernel-loop leg: %d iterations with the set on, %d cleared):" % (args.steps, args.steps))
    with tempfile.TemporaryDirectory() as d:
        args_loop = argparse.Namespace(steps=args.steps, reps=args.reps)
        if not child("kernel-loop", args_loop, out, prefix=(prof, "--kernel-trace", "-d", d, "-o", "p", "--")):
            return 1
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "kernel-table", "--kernel-db", d], stdout=subprocess.PIPE, text=True, cwd=ROOT)
        for line in r.stdout.splitlines():
            out(line)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
