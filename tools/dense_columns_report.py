"""What the dense-column split of the sparse factor buys and costs on the device.

  * Netlib FIT1P, SEBA, ISRAEL in standard form (tests/golden/netlib) and in general form with native bounds (tests/golden/general):
    status, iterations, device ms per iteration (ipm_stats.solve_ms / iterations) and the final residuals, for the unsplit
    factor="auto" handle against the split handle (factor="sparse", dense_cols=analysis.dense_columns(A)), each with refine = 0 and 1
    (a split handle runs at least two refinement rounds of its own, whatever is asked: its two lines are the same run twice).
    Mehrotra's start on the device, tol 1e-8 (general form: e3 = 1e-6, cap 999, what new_interior_sparse runs).
  * Per-stage cost of the extra launches: the phase timers (ipm_set_profiling(2)) of the split handle against a handle on the same
    A with the dense columns EMPTIED -- the same sparse factor L without a split -- so the differences of the "factor" and
    "trisolve" phases are the split's launches per factorization and per iteration's solves.
  * Large LPs: workloads.block_angular_lp at m in {4096, 16384} with k in {8, 64} linking columns, --steps iterations from the
    reference start on the split handle against the dense-tile path (factor="dense"), ms per iteration from HIP events.

    python tools/dense_columns_report.py [--no-netlib] [--no-stages] [--no-large] [--steps N] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interiorpointmethod_amd import analysis, api  # noqa: E402
from interiorpointmethod_amd import general_form as G  # noqa: E402
from interiorpointmethod_amd.handle import IpmSolver  # noqa: E402
from interiorpointmethod_amd.matio import load_npz_problem  # noqa: E402
from interiorpointmethod_amd.workloads import block_angular_lp  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("FIT1P", "SEBA", "ISRAEL")


class Tee:
    def __init__(self, path):
        self.fh = open(path, "w") if path else None

    def __call__(self, line=""):
        print(line, flush=True)
        if self.fh:
            self.fh.write(line + "\n")
            self.fh.flush()


def load_general(name):
    z = np.load(os.path.join(GOLD, "general", name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    F = G.native_form(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                      bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])
    return sparse.csc_matrix(F.A), F.b, F.c, F.u


def load_standard(name):
    A, b, c, _, _ = load_npz_problem(os.path.join(GOLD, "netlib", name + ".npz"))
    return sparse.csc_matrix(A, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel(), None


def netlib(out):
    out("Netlib: unsplit factor=\"auto\" against the split (factor=\"sparse\", dense_cols=dense_columns(A)); Mehrotra's start on the device")
    out("%-8s %-9s %5s %3s | %-6s %6s | %-9s %4s %9s %9s %9s" % ("file", "form", "m", "k", "handle", "refine", "status", "it", "ms/it", "rp", "rd"))
    for form, load, kw in (("standard", load_standard, dict(tol=1e-8, max_iter=300)), ("general", load_general, dict(tol=1e-8, tol_gap=1e-6, max_iter=999))):
        for name in NAMES:
            A, b, c, u = load(name)
            cols = analysis.dense_columns(A)
            for tag, hkw in (("unsplit", {}), ("split", dict(factor="sparse", dense_cols=cols))):
                for k in (0, 1):
                    try:
                        info = api.solve_with_info(A, b, c, ub=u, start="mehrotra", device_start=True, refine=k, **kw, **hkw)[3]
                        line = "%-9s %4d %9.4f %9.2e %9.2e" % (info["status_name"], info["iterations"], info["solve_ms"] / max(1, info["iterations"]),
                                                               info["rp"], info["rd"])
                        tag2 = "%s/%s" % (tag, info["factor_path"][0])
                    except Exception as e:          # a refusal is a line of the table
                        line, tag2 = "%s: %s" % (type(e).__name__, str(e)[:60]), tag
                    out("%-8s %-9s %5d %3d | %-9s %3d | %s" % (name, form, A.shape[0], cols.size, tag2, k, line))
    out()


def stages(out, steps):
    out("Per-stage cost of the split's launches (phase timers over %d iterations from the reference start; same L with and without)" % steps)
    out("%-8s %5s %3s | %21s | %21s | %9s %9s" % ("file", "m", "k", "factor ms/it  no/split", "trisolve ms/it no/split", "+factor", "+solves"))
    cases = [(nm,) + load_standard(nm)[:3] for nm in ("FIT1P", "SEBA")]
    for m, k in ((4096, 8), (4096, 64)):
        A, b, c, _ = block_angular_lp(m, 64, k, seed=1)
        cases.append(("BA%dk%d" % (m, k), A, b.ravel(), c.ravel()))
    for name, A, b, c in cases:
        cols = analysis.dense_columns(A)
        ph = []
        for M, dc in ((analysis.without_columns(A, cols), None), (A, cols)):
            with IpmSolver(M, b, c, factor="sparse", dense_cols=dc) as sv:
                sv.init_state(1.0)
                sv.iterate(2)
                sv.init_state(1.0)
                sv.set_profiling(2)
                sv.iterate(steps)
                ph.append(sv.phase_ms())
        out("%-8s %5d %3d | %10.4f %10.4f | %10.4f %10.4f | %9.4f %9.4f" % (name, A.shape[0], cols.size, ph[0]["factor"], ph[1]["factor"],
            ph[0]["trisolve"], ph[1]["trisolve"], ph[1]["factor"] - ph[0]["factor"], ph[1]["trisolve"] - ph[0]["trisolve"]))
    out()


def large(out, steps):
    import torch
    out("Block-angular LPs (workloads.block_angular_lp, blocks of 64 rows): %d iterations from the reference start, ms per iteration" % steps)
    out("%6s %3s | %12s %12s %8s | %s" % ("m", "k", "dense tiles", "split", "gain", "nnz(L) with the split"))
    for m in (4096, 16384):
        for k in (8, 64):
            A, b, c, cols = block_angular_lp(m, 64, k, seed=1)
            b, c = b.ravel(), c.ravel()
            ms, nnz = [], 0
            for hkw in (dict(factor="dense", reorder=False), dict(factor="sparse", dense_cols=cols)):
                with IpmSolver(A, b, c, **hkw) as sv:
                    sv.init_state(1.0)
                    sv.iterate(2)
                    sv.init_state(1.0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    sv.iterate(steps)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1) / steps)
                    if sv.dense_cols is not None:
                        nnz = sv.dense_split_info()["factor_entries"]
            out("%6d %3d | %12.3f %12.3f %7.1fx | %d" % (m, k, ms[0], ms[1], ms[0] / ms[1], nnz))
    out()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-netlib", action="store_true")
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_columns_report.txt"))
    a = ap.parse_args()
    import torch
    out = Tee(a.out)
    out("dense-column split report -- device: %s" % torch.cuda.get_device_name(0))
    out()
    if not a.no_netlib:
        netlib(out)
    if not a.no_stages:
        stages(out, a.steps)
    if not a.no_large:
        large(out, a.steps)


if __name__ == "__main__":
    main()
