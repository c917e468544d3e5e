#!/usr/bin/env python3
"""Throughput of small factor-model QPs on the one-workgroup path (IPM_FLAG_SMALL_FREE): one solve_small_factor_qp_batch call against
the loop over solve_factor_qp on multi-kernel handles -- the only way such a problem had before the flag.

Workloads:
    sweep     a risk-aversion sweep of a 1 x 64 portfolio with 8 factors: min -mu.x + lambda/2 x.(diag(sigma^2) + B B^T) x, 1^T x = 1,
              0 <= x <= 0.25, one problem per lambda of a log grid over 1e-2 .. 1e2 (256 by default)
    factor    distinct workloads.factor_qp problems of 20 x 130 with 16 factors (1024 by default)
Each is timed two ways, host wall clock of the whole call (handle creation, upload, solve, read-back, close: what a caller pays):
    batch     ONE solve_small_factor_qp_batch call
    loop      solve_factor_qp(csc A, b, c, F, g, ub) per problem, the default multi-kernel path
One warm-up, then --reps repetitions (at least five): median, min, max; beside each, the part of the last repetition spent solving
(the batch's one device interval; the loop's host time inside solve()).  Handle creation dominates both front ends, so each workload
is also timed with the handles LIVE (created once, init_state outside the clock): one solve_small_batch_solvers call over
free_small handles against the loop of solve() over multi-kernel handles.  --only loop runs the loops alone and needs nothing this
feature adds, so the same file times them in a checkout of the parent commit (--label parent).
Also: a lone problem of each workload on both paths (device time of the solve, info["solve_ms"], and the iterations), and the device
time per iteration of the Free variant of the kernel against the Quad variant at the same shape: the augmented problem of one handle
with its free set, cleared, and set again (cleared, the k columns are barrier columns: another problem, the same shape and list).

    python tools/small_factor_qp_bench.py [--reps 5] [--out profiles/small_factor_qp_batch.txt] [--only loop --label parent]

--out appends, so the lines of both commits can share a file.  One process, one GPU.  Run it under a time limit of its own."""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import interiorpointmethod_amd as ipm  # noqa: E402
from interiorpointmethod_amd.workloads import factor_qp  # noqa: E402


def portfolio_sweep(n, assets=64, factors=8, seed=3):
    """-> (problems (A, b, c, F, g), ub): one problem per risk aversion lambda; lambda scales diag(g) and F F^T alike."""
    rng = np.random.default_rng(seed)
    mu, sigma = rng.uniform(0.02, 0.12, assets), rng.uniform(0.05, 0.4, assets)
    B = rng.standard_normal((assets, factors)) * 0.1
    A = sparse.csc_matrix(np.ones((1, assets)))
    lam = np.logspace(-2, 2, n) if n > 1 else np.array([1.0])
    return [(A, np.ones(1), -mu, np.sqrt(l) * B, l * sigma * sigma) for l in lam], [np.full(assets, 0.25)] * len(lam)


def factor_problems(n, m=20, cols=130, k=16):
    out, ub = [], []
    for i in range(n):
        A, b, c, g, F, u, xs, ys = factor_qp(m, cols, k, 100 + i, bounded=True)
        out.append((sparse.csc_matrix(A), b, c, F, g)); ub.append(u)
    return out, ub


def timed(fn, reps):
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        t.append(time.perf_counter() - t0)
    t = np.asarray(t[1:]) * 1e3                      # the first one is the warm-up
    return (float(np.median(t)), float(t.min()), float(t.max())), res


def loop(problems, ub, max_iter, **kw):
    return [ipm.solve_factor_qp(A, b, c, F, g=g, ub=u, tol=1e-8, max_iter=max_iter, **kw) for (A, b, c, F, g), u in zip(problems, ub)]


def summary(res):
    return sum(r[3]["iterations"] for r in res), sum(r[3]["status"] == 1 for r in res)


def measure(label, problems, ub, reps, max_iter, only, out):
    n = len(problems)
    line = "%-18s %5d QPs" % (label, n)
    bt = None
    if only in ("both", "batch"):
        bt, res = timed(lambda: ipm.solve_small_factor_qp_batch(problems, tol=1e-8, ub=ub, max_iter=max_iter), reps)
        assert all(r[3]["quadratic_path"] == "one-workgroup" for r in res)
        line += " | batch %6d iterations %5d converged %10.3f ms (min %10.3f max %10.3f) %9.0f QPs/s, of it the device time of the one solve call %9.3f ms" \
                % (summary(res) + bt + (1e3 * n / bt[0], res[0][3]["solve_ms"]))
    if only in ("both", "loop"):
        lp, res = timed(lambda: loop(problems, ub, max_iter), reps)
        assert all(r[3]["quadratic_path"] == "multi-kernel" for r in res)
        line += " | multi-kernel loop %6d iterations %5d converged %10.3f ms (min %10.3f max %10.3f), of it inside the solves %9.3f ms" \
                % (summary(res) + lp + (1e3 * sum(r[3]["solve_seconds"] for r in res),))
        if bt:
            line += " | loop / batch %7.2f (min loop / max batch %7.2f)" % (lp[0] / bt[0], lp[1] / bt[2])
    out(line)


def live(label, problems, ub, reps, max_iter, only, out):
    """The solves alone, handles created once and live across the repetitions (a caller that re-solves: new c, new bounds, a warm
    start): ONE solve_small_batch_solvers call over free_small handles against the loop of solve() over multi-kernel handles; every
    repetition resets the states with init_state first, outside the clock."""
    forms = [ipm.factor_qp_form(A, b, c, g, F, u) for (A, b, c, F, g), u in zip(problems, ub)]
    line = "%-18s %5d QPs, handles live" % (label, len(problems))

    def run(svs, fn):
        t = []
        for _ in range(reps + 1):
            for sv in svs:
                sv.init_state(1.0)
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        t = np.asarray(t[1:]) * 1e3
        return float(np.median(t)), float(t.min()), float(t.max())
    bt = None
    for what, kw in (("batch", {"free_small": True}), ("loop", {})):
        if only not in ("both", what):
            continue
        svs = []
        try:
            svs = [ipm.IpmSolver(A_, b_, c_, ub=u_, quad=g_, free=fr, **kw) for A_, b_, c_, g_, u_, fr in forms]
            assert all(ipm.small_batch_eligible(sv) == (what == "batch") for sv in svs)
            if what == "batch":
                bt = run(svs, lambda: ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=max_iter))
                line += " | batch %6d iterations %10.3f ms (min %10.3f max %10.3f)" % ((sum(sv.stats["iterations"] for sv in svs),) + bt)
            else:
                lp = run(svs, lambda: [sv.solve(tol=1e-8, max_iter=max_iter) for sv in svs])
                line += " | multi-kernel loop %6d iterations %10.3f ms (min %10.3f max %10.3f)" % ((sum(sv.stats["iterations"] for sv in svs),) + lp)
                if bt:
                    line += " | loop / batch %7.2f (min loop / max batch %7.2f)" % (lp[0] / bt[0], lp[1] / bt[2])
        finally:
            for sv in svs:
                sv.close()
    out(line)


def lone(label, problem, u, reps, max_iter, out):
    A, b, c, F, g = problem
    cols = []
    for what, kw in (("one-workgroup", {"free_small": True}), ("multi-kernel", {})):
        ms, wall = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            info = ipm.solve_factor_qp(A, b, c, F, g=g, ub=u, tol=1e-8, max_iter=max_iter, **kw)[3]
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(info["solve_ms"])
        assert info["quadratic_path"] == what and info["status"] == 1
        ms, wall = np.asarray(ms[1:]), np.asarray(wall[1:])
        cols.append("%s %d iterations, device %8.3f ms (min %8.3f max %8.3f), whole call %8.3f ms (min %8.3f max %8.3f)"
                    % (what, info["iterations"], np.median(ms), ms.min(), ms.max(), np.median(wall), wall.min(), wall.max()))
    out("%-18s lone problem: %s" % (label, " | ".join(cols)))


def per_iteration(label, problem, u, reps, steps, out):
    """Device time of `steps` iterations in ONE launch of the small loop from the reference start (ipm_iterate: no stop test ends it) on
    the augmented problem of one handle: with its free set (the Free variant), cleared (the Quad variant), and set again."""
    A, b, c, F, g = problem
    A_, b_, c_, g_, u_, free = ipm.factor_qp_form(A, b, c, g, F, u)
    with ipm.IpmSolver(A_, b_, c_, ub=u_, quad=g_, free=free, free_small=True) as sv:
        assert ipm.small_batch_eligible(sv)
        t = {}
        for what, fs in (("Free", free), ("Quad", None), ("Free again", free)):
            sv.set_free(fs)
            ms = []
            for _ in range(reps + 1):
                sv.init_state(1.0)
                ms.append(sv.iterate(steps)["solve_ms"])
            t[what] = np.asarray(ms[1:]) * 1e3 / steps
    out("%-18s us per iteration, %d iterations in one launch, %d x %d augmented: %s"
        % (label, steps, A_.shape[0], A_.shape[1], " | ".join("%s %8.2f (min %8.2f max %8.2f)" % (k, np.median(v), v.min(), v.max()) for k, v in t.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", type=int, default=256, help="risk aversions of the portfolio sweep")
    ap.add_argument("--factor", type=int, default=1024, help="problems of the 20 x 130, k = 16 workload")
    ap.add_argument("--only", default="both", choices=["both", "batch", "loop"])
    ap.add_argument("--label", default="this", help="what the lines are tagged with (parent: the loop timed in a checkout of the parent commit)")
    a = ap.parse_args()
    reps = max(5, a.reps)
    fh = open(a.out, "a") if a.out else None

    def out(s):                                      # the record is written as the results arrive
        s = "%-7s %s" % (a.label, s) if not s.startswith("#") else s
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    import torch
    out("# [%s] small factor-model QP batch: one solve_small_factor_qp_batch call against the loop over solve_factor_qp on multi-kernel handles" % a.label)
    out("# [%s] device: %s; host wall time of the whole call in ms (handles created and closed inside), median of %d repetitions after one warm-up; tol 1e-8, cap %d"
        % (a.label, torch.cuda.get_device_name(0), reps, a.max_iter))
    sweep, sweep_ub = portfolio_sweep(a.sweep)
    fact, fact_ub = factor_problems(a.factor)
    measure("sweep 1x64 k=8", sweep, sweep_ub, reps, a.max_iter, a.only, out)
    measure("factor 20x130 k=16", fact, fact_ub, reps, a.max_iter, a.only, out)
    live("sweep 1x64 k=8", sweep, sweep_ub, reps, a.max_iter, a.only, out)
    live("factor 20x130 k=16", fact, fact_ub, reps, a.max_iter, a.only, out)
    if a.only == "both":
        lone("sweep 1x64 k=8", sweep[len(sweep) // 2], sweep_ub[0], reps, a.max_iter, out)
        lone("factor 20x130 k=16", fact[0], fact_ub[0], reps, a.max_iter, out)
        out("# [%s] the Free variant of the one-workgroup kernel against the Quad variant on the same handle (device time, median of %d after one warm-up)" % (a.label, reps))
        per_iteration("sweep 1x64 k=8", sweep[len(sweep) // 2], sweep_ub[0], reps, 8, out)
        per_iteration("factor 20x130 k=16", fact[0], fact_ub[0], reps, 8, out)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
