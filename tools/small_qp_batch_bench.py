#!/usr/bin/env python3
"""Throughput of small separable QPs on the one-workgroup path (IPM_FLAG_SMALL_QUADRATIC): one ipm_solve_small_batch call against a
loop of ipm_solve over the same flagged handles, and against a loop over unflagged handles -- the multi-kernel path, the only way a
small QP had before the flag.

Workloads: N distinct workloads.separable_qp problems of 50 x 130 (bounded + mixed) for N in 1, 16, 64, 256, 1024, and one
portfolio sweep: m = 1, 1^T x = 1, 0 <= x <= u, c = -(expected returns), g = lambda sigma^2 over a grid of N risk aversions lambda
(the natural caller, and the nt = 1 edge of the kernel).  Per workload the handles are created once; every repetition resets the
states with init_state, then times (host wall clock, the call returns with everything complete) ONE batch call, the loop of solve()
over the flagged handles, or the loop over the unflagged ones.  One warm-up, then --reps repetitions (at least five): median, min,
max.  The three columns of a row are measured in one process, one after the other.  Last: the device time per iteration of the QP
variant of the kernel against its LP twin, on one handle with the term set, cleared and set again.

    python tools/small_qp_batch_bench.py [--reps 7] [--out profiles/small_qp_batch.txt]

One process, one GPU.  Run it under a time limit of its own."""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd.solver import IpmSolver, small_batch_eligible, solve_small_batch_solvers  # noqa: E402
from interiorpointmethod_amd.workloads import separable_qp  # noqa: E402


def qp_problems(n):
    out = []
    for k in range(n):
        A, b, c, g, u, xs, ys = separable_qp(50, 130, 100 + k, bounded=True, mixed=True)
        out.append((sparse.csc_matrix(A), b, c, g, u))
    return out


def portfolio_sweep(n, assets=64, seed=3):
    """min -mu.x + lambda/2 x.diag(sigma^2) x, 1^T x = 1, 0 <= x <= 0.25: one problem per lambda of a log grid over 1e-2 .. 1e2."""
    rng = np.random.default_rng(seed)
    mu, sigma = rng.uniform(0.02, 0.12, assets), rng.uniform(0.05, 0.4, assets)
    A = sparse.csc_matrix(np.ones((1, assets)))
    lam = np.logspace(-2, 2, n) if n > 1 else np.array([1.0])
    return [(A, np.ones(1), -mu, l * sigma * sigma, np.full(assets, 0.25)) for l in lam]


def timed(svs, fn, reps):
    t = []
    for _ in range(reps + 1):
        for sv in svs:
            sv.init_state(1.0)
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t = np.asarray(t[1:]) * 1e3                      # the first one is the warm-up
    return float(np.median(t)), float(t.min()), float(t.max())


def measure(label, problems, reps, max_iter, out):
    small = [IpmSolver(A, b, c, ub=u, quad=g, quad_small=True) for A, b, c, g, u in problems]
    multi = []
    try:
        assert all(small_batch_eligible(sv) for sv in small)
        bt = timed(small, lambda: solve_small_batch_solvers(small, max_iter=max_iter), reps)
        iters = sum(sv.stats["iterations"] for sv in small)
        conv = sum(sv.stats["status"] == 1 for sv in small)
        lp = timed(small, lambda: [sv.solve(tol=1e-8, max_iter=max_iter) for sv in small], reps)
        assert iters == sum(sv.stats["iterations"] for sv in small)          # the same solves
        multi = [IpmSolver(A, b, c, ub=u, quad=g) for A, b, c, g, u in problems]
        assert not any(small_batch_eligible(sv) for sv in multi)
        mk = timed(multi, lambda: [sv.solve(tol=1e-8, max_iter=max_iter) for sv in multi], reps)
        mk_iters = sum(sv.stats["iterations"] for sv in multi)
    finally:
        for sv in small + multi:
            sv.close()
    out("%-16s %5d QPs %6d iterations (multi-kernel %6d) %5d converged | batch %9.3f ms (min %9.3f max %9.3f) | small loop %9.3f ms (min %9.3f max %9.3f) | "
        "multi-kernel loop %9.3f ms (min %9.3f max %9.3f) | small loop / batch %6.2f | multi-kernel loop / batch %7.2f | %9.0f QPs/s batch"
        % (label, len(problems), iters, mk_iters, conv, bt[0], bt[1], bt[2], lp[0], lp[1], lp[2], mk[0], mk[1], mk[2], lp[0] / bt[0], mk[0] / bt[0],
           1e3 * len(problems) / bt[0]))


def per_iteration(label, problem, reps, steps, out):
    """Device time of `steps` iterations in ONE launch of the small loop from the reference start (ipm_iterate: no stop test ends it),
    with the term and, on the same handle, with the term cleared: the QP variant of the kernel against its LP twin."""
    A, b, c, g, u = problem
    with IpmSolver(A, b, c, ub=u, quad=g, quad_small=True) as sv:
        assert small_batch_eligible(sv)
        t = {}
        for what, term in (("QP", g), ("LP", None), ("QP again", g)):
            sv.set_quadratic(term)
            ms = []
            for _ in range(reps + 1):
                sv.init_state(1.0)
                ms.append(sv.iterate(steps)["solve_ms"])
            t[what] = np.asarray(ms[1:]) * 1e3 / steps
    out("%-16s us per iteration, %d iterations in one launch: %s"
        % (label, steps, " | ".join("%s %8.2f (min %8.2f max %8.2f)" % (k, np.median(v), v.min(), v.max()) for k, v in t.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    ap.add_argument("--sweep", type=int, default=256, help="risk aversions of the portfolio sweep")
    a = ap.parse_args()
    reps = max(5, a.reps)
    fh = open(a.out, "w") if a.out else None

    def out(s):                                      # the record is written as the results arrive
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    import torch
    out("# small QP batch: one ipm_solve_small_batch call against a loop of ipm_solve over the same flagged handles (small loop) and over unflagged handles (multi-kernel loop)")
    out("# device: %s; wall time per call in ms, median of %d repetitions after one warm-up, states reset by init_state; tol 1e-8, cap %d; all handles of a row live at once"
        % (torch.cuda.get_device_name(0), reps, a.max_iter))
    for n in (int(v) for v in a.sizes.split(",")):
        measure("QP 50x130 x %d" % n, qp_problems(n), reps, a.max_iter, out)
    measure("portfolio 1x64", portfolio_sweep(a.sweep), reps, a.max_iter, out)
    out("# the QP variant of the one-workgroup kernel against its LP twin on the same handle (device time, median of %d after one warm-up)" % reps)
    per_iteration("QP 50x130", qp_problems(1)[0], reps, 8, out)
    per_iteration("portfolio 1x64", portfolio_sweep(1)[0], reps, 8, out)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
