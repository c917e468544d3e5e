#!/usr/bin/env python3
"""What the bounded twins of the lockstep batch buy (IPM_FLAG_LOCKSTEP_BOUNDS): the general-form fixtures of
tests/golden/general in NATIVE form (general_form.native_form: 0 <= x <= u inside the Newton system) whose row count is in the
lockstep range, all of them, bounded and unbounded mixed as a user would have them, solved on one GPU

    lockstep leg (default)    batch.run_batch(problems, lockstep=True, workers=8, start="mehrotra") over (A, b, c, ub) tuples;
    --one-at-a-time           batch.solve_shard(workers=8) with a solve function of this file that calls solve_with_info(..., ub=,
                              start="mehrotra", device_start=True, concurrent=True): the worker streams of solve_shard, four chains on
                              four hardware queues.  This leg uses nothing newer than solve_with_info(ub=), so it also runs from a
                              checkout of the commit before the bounded twins -- which is where the comparison is meant to run it.

Both legs: tol 1e-8, gap tolerance 1e-6, at most 999 iterations (the settings of general_form.new_interior_sparse).  One warm-up
run, then --runs timed runs in the same process; per run LPs/s, wall seconds and the converged count, then the per-LP status,
iteration count and objective (+ NativeForm.offset: the original problem's) of the last run.

    python tools/lockstep_bounds_report.py [--one-at-a-time] [--runs 5] [--max-rows 1600] [--out FILE (appended to)]

One process, one GPU.  Run it under a time limit of its own."""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd import batch  # noqa: E402
from interiorpointmethod_amd import general_form as G  # noqa: E402
from interiorpointmethod_amd.api import solve_with_info  # noqa: E402

GEN = os.path.join(ROOT, "tests", "golden", "general")
STOP = dict(tol=1e-8, tol_gap=1e-6, max_iter=999)


def load(name):
    z = np.load(os.path.join(GEN, name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"]), float(z["netlib_optimum"])


def problems(max_rows):
    """(names, (A, b, c, u) tuples, offsets, Netlib optima) of every fixture whose native form has 129 .. max_rows rows."""
    names, probs, offsets, optima = [], [], [], []
    for f in sorted(os.listdir(GEN)):
        if not f.endswith(".npz"):
            continue
        try:
            args, opt = load(f[:-4])
            F = G.native_form(**args)
        except (ValueError, KeyError):              # a free variable, or a fixture without a general form
            continue
        if 128 < F.A.shape[0] <= max_rows:
            names.append(f[:-4]); probs.append((F.A, F.b, F.c, F.u)); offsets.append(F.offset); optima.append(opt)
    return names, probs, offsets, optima


def one_at_a_time(problem, device=0, **_):
    A, b, c, u = problem
    return solve_with_info(A, b, c, ub=u, device=device, start="mehrotra", device_start=True, concurrent=True, **STOP)[3]


def run(probs, lockstep):
    t0 = time.perf_counter()
    if lockstep:
        rec, _ = batch.run_batch(probs, lockstep=True, workers=8, start="mehrotra", **STOP)
    else:
        rec = batch.solve_shard(probs, list(range(len(probs))), device=0, solve_fn=one_at_a_time, workers=8)
    return rec, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-at-a-time", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=1600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quiet-table", action="store_true", help="leave the per-LP table out")
    a = ap.parse_args()
    fh = open(a.out, "a") if a.out else None

    def out(s):
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    import torch
    names, probs, offsets, optima = problems(a.max_rows)
    bounded = sum(1 for p in probs if np.isfinite(p[3]).any())
    leg = "one-at-a-time (solve_with_info(ub=) on 8 worker streams)" if a.one_at_a_time else "lockstep (run_batch(lockstep=True, workers=8))"
    out("# %s | %s | %d native-form LPs of 129 .. %d rows, %d with finite bounds | start=mehrotra tol 1e-8 gap 1e-6 cap 999 | one warm-up run first"
        % (leg, torch.cuda.get_device_name(0), len(probs), a.max_rows, bounded))
    run(probs, not a.one_at_a_time)
    rec = None
    for k in range(a.runs):
        rec, secs = run(probs, not a.one_at_a_time)
        out("run %d: %7.2f LPs/s  %7.3f s wall  %d of %d converged" % (k + 1, len(probs) / secs, secs, int((rec[:, 1] == 1.0).sum()), len(probs)))
    if rec is not None and not a.quiet_table:
        out("# per LP (last run): name rows cols bounds status iterations objective+offset | Netlib optimum")
        for k, nm in enumerate(names):
            A, u = probs[k][0], probs[k][3]
            out("%-10s %5d %6d %5d  %d %4d  %.12e | %.12e" % (nm, A.shape[0], A.shape[1], int(np.isfinite(u).sum()), int(rec[k, 1]), int(rec[k, 2]),
                                                            rec[k, 3] + offsets[k], optima[k]))
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
