#!/usr/bin/env python3
"""Throughput of the small-LP batch (ipm_solve_small_batch) against a loop of ipm_solve over the same handles.

Workloads: N copies of AFIRO for N in 1, 16, 64, 256, 1024, and the mixed set of every file of tests/golden/netlib/ with at most 128
rows that the fused small-LP path serves.  Per workload the handles are created once; every repetition resets the states with
init_state, then times (host wall clock, the call returns with everything complete) either ONE batch call or the loop of
ipm_solve, which is what a caller had before the batch existed.  One warm-up, then --reps repetitions (at least five): median, min, max.

    python tools/small_batch_bench.py [--reps 7] [--out profiles/small_batch_throughput.txt]

One process, one GPU; reads only tests/golden/.  Run it under a time limit of its own."""
import argparse
import glob
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd.solver import IpmSolver, small_batch_eligible, solve_small_batch_solvers  # noqa: E402

NETLIB = os.path.join(ROOT, "tests", "golden", "netlib")


def load(name):
    d = np.load(os.path.join(NETLIB, name + ".npz"))
    A = sparse.csc_matrix((d["data"], d["indices"], d["indptr"]), shape=tuple(int(v) for v in d["shape"]))
    return A, np.asarray(d["b"], dtype=np.float64).ravel(), np.asarray(d["c"], dtype=np.float64).ravel()


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
    svs = [IpmSolver(A, b, c) for A, b, c in problems]
    try:
        bt = timed(svs, lambda: solve_small_batch_solvers(svs, max_iter=max_iter), reps)
        iters = sum(sv.stats["iterations"] for sv in svs)
        conv = sum(sv.stats["status"] == 1 for sv in svs)
        lp = timed(svs, lambda: [sv.solve(tol=1e-8, max_iter=max_iter) for sv in svs], reps)
        assert iters == sum(sv.stats["iterations"] for sv in svs)          # the same solves
    finally:
        for sv in svs:
            sv.close()
    out("%-14s %5d LPs %7d iterations %5d converged | batch %9.3f ms (min %9.3f max %9.3f) | loop %9.3f ms (min %9.3f max %9.3f) | loop / batch %6.2f | %9.0f LPs/s batch"
        % (label, len(problems), iters, conv, bt[0], bt[1], bt[2], lp[0], lp[1], lp[2], lp[0] / bt[0], 1e3 * len(problems) / bt[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    a = ap.parse_args()
    reps = max(5, a.reps)
    fh = open(a.out, "w") if a.out else None

    def out(s):                                      # the record is written as the results arrive
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    import torch
    out("# small-LP batch: one ipm_solve_small_batch call against a loop of ipm_solve over the same handles")
    out("# device: %s; wall time per call in ms, median of %d repetitions after one warm-up, states reset by init_state; tol 1e-8, cap %d"
        % (torch.cuda.get_device_name(0), reps, a.max_iter))
    afiro = load("AFIRO")
    for n in (int(v) for v in a.sizes.split(",")):
        measure("AFIRO x %d" % n, [afiro] * n, reps, a.max_iter, out)
    mixed, names, dropped = [], [], []
    for f in sorted(glob.glob(os.path.join(NETLIB, "*.npz"))):
        if int(np.load(f)["shape"][0]) <= 128:
            name = os.path.basename(f)[:-4]
            lp = load(name)
            with IpmSolver(*lp) as sv:               # the library decides (product list within its cap)
                on_path = small_batch_eligible(sv)
            if on_path:
                mixed.append(lp); names.append(name)
            else:
                dropped.append(name)
    out("# mixed Netlib = %s%s" % (" ".join(names), ("; not on the small path, left out: " + " ".join(dropped)) if dropped else ""))
    measure("mixed Netlib", mixed, reps, a.max_iter, out)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
