"""Time the device LU (ipm_lu_solve) at the given orders and panel widths: wall time of each call (upload, factorization,
substitution, download) and the scaled backward error.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/lu_bench.py ...` run.

    python tools/lu_bench.py --n 2048 8192 20480 --nb 128 64 --reps 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import interiorpointmethod_amd as ipm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2048, 8192, 20480])
    ap.add_argument("--nb", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--nrhs", type=int, default=1)
    args = ap.parse_args()
    for n in args.n:
        rng = np.random.default_rng(n)
        A = rng.standard_normal((n, n))
        b = rng.standard_normal((n, args.nrhs))
        flops = 2.0 * n ** 3 / 3.0
        for nb in args.nb:
            os.environ["IPM_LU_NB"] = str(nb)
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                x = ipm.lu_solve(A, b)
                times.append(time.perf_counter() - t0)
            r = np.abs(A @ x - b).max()
            be = r / (np.abs(A).sum(axis=1).max() * np.abs(x).max() * n * np.finfo(float).eps)
            print(json.dumps({"n": n, "nb": nb, "nrhs": args.nrhs, "wall_s": [round(t, 4) for t in times],
                              "factor_gflop": round(flops / 1e9, 1), "backward_error": float("%.3g" % be)}), flush=True)


if __name__ == "__main__":
    main()
