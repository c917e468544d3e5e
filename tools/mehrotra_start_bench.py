#!/usr/bin/env python
"""Time of Mehrotra's starting point alone, from the call to the state being resident on the device: the host recipe
set_state(*mehrotra_start()) against the device start init_state_mehrotra() on the same handle, and for the small path
init_small_batch_mehrotra over N handles against N single calls.  Both variants alternate inside one run; warm-up first, then the
median (and min / max) of the repeats of a host clock around calls that end in a device synchronisation.

    python tools/mehrotra_start_bench.py [--repeats 30] [--batch 1000] [--out profiles/mehrotra_start.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import interiorpointmethod_amd as ipm                       # noqa: E402
from interiorpointmethod_amd.matio import load_npz_problem  # noqa: E402


def load(name):
    A, b, c, _, _ = load_npz_problem(os.path.join(ROOT, "tests", "golden", "netlib", name + ".npz"))
    return A, b, c


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(label, ms):
    return "%-44s median %9.3f ms   min %9.3f   max %9.3f   (n = %d)" % (label, statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = ["# Mehrotra's starting point alone (call -> state resident), ms per start; host recipe and device start alternate in one run"]

    def out(s):
        rows.append(s)
        print(s, flush=True)

    for name in ("AFIRO", "SC205", "SCAGR25"):
        A, b, c = load(name)
        with ipm.IpmSolver(A, b, c) as sv:
            host = lambda: sv.set_state(*sv.mehrotra_start())          # noqa: E731
            dev = lambda: sv.init_state_mehrotra()                     # noqa: E731
            for _ in range(3):
                host(); dev()
            th, td = [], []
            for _ in range(args.repeats):                              # alternate: both see the same neighbours on the machine
                th += timed(host, 1)
                td += timed(dev, 1)
            out(line("%s %dx%d host recipe" % (name, sv.m, sv.n), th))
            out(line("%s %dx%d device start" % (name, sv.m, sv.n), td))
    A, b, c = load("AFIRO")
    svs = [ipm.IpmSolver(A, b, c) for _ in range(args.batch)]
    try:
        loop = lambda: [sv.init_state_mehrotra() for sv in svs]        # noqa: E731
        one = lambda: ipm.init_small_batch_mehrotra(svs)               # noqa: E731
        hostloop = lambda: [sv.set_state(*sv.mehrotra_start()) for sv in svs]      # noqa: E731
        loop(); one()
        reps = max(3, args.repeats // 6)
        tl, tb = [], []
        for _ in range(reps):
            tl += timed(loop, 1)
            tb += timed(one, 1)
        th = timed(hostloop, 2)
        out(line("%d x AFIRO host recipe, one by one" % args.batch, th))
        out(line("%d x AFIRO init_state_mehrotra, one by one" % args.batch, tl))
        out(line("%d x AFIRO init_small_batch_mehrotra" % args.batch, tb))
        ref = [np.concatenate([v.ravel() for v in sv.get_state()]) for sv in svs[:3]]
        assert all(np.array_equal(ref[0], r) for r in ref)
    finally:
        for sv in svs:
            sv.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
