"""The cells of tests/test_gpu_variant_bits.py and tools/record_variant_bits.py: one solve per problem class and launch path, each
reduced to (iterations, status, sha256 of the bytes of x, y, s[, w, z]).  The fixture tests/golden/variant_bits_parent.json holds
what a build of the commit BEFORE the class-variant tables computed; the test holds the current build to the same bits.

Classes: the twelve legal combinations of B (upper bounds), D (infeasibility tests), Q (quadratic term), F (free columns; needs Q).
Problem data, from the seeded generator workloads.synthetic_lp(m, n, seed): its A (for a sparse cell only the entries with |a| >= 0.6,
plus one per column so that none is empty), b = A 1 and c' = |c| + 0.5, so x = 1 is strictly feasible and (y, s) = (0, c') is dual
feasible.  B: every fourth column (5 of 20) gets u = 2.  F: columns 0, 4, 8 are free.  Q: g > 0 on those three and on columns 1, 5,
9, 13.  Every solve starts from init_state(1.0).

Paths (`cells()`): "dense" 8 x 20 dense A, the multi-kernel path; "small" the same data as a sparse A, the one-workgroup kernel;
"batch" those twelve sparse problems in ONE ipm_solve_small_batch call; "lockstep" (classes -, B, D, BD) two sparse 130 x 300
problems in one lockstep batch; "large" (classes -, B, BQF) dense 2304 x 4608, 18 blocks -- past the 16 at which the residual
stream exists, the only path that launches the scaling step -- stopped by max_iter = 3; "start" (classes -, B) Mehrotra's start on
the dense and the small path, and "start-batch" both small ones in one ipm_init_small_batch_mehrotra call."""
import hashlib

import numpy as np
from scipy import sparse

CLASSES = ("-", "B", "D", "BD", "Q", "BQ", "QF", "BQF", "DQ", "BDQ", "DQF", "BDQF")
LOCKSTEP_CLASSES = ("-", "B", "D", "BD")
LARGE_CLASSES = ("-", "B", "BQF")
START_CLASSES = ("-", "B")
SMALL_SHAPE, LOCKSTEP_SHAPE, LARGE_SHAPE = (8, 20), (130, 300), (2304, 4608)
SEED = 7                                # every cell reaches status 1 with it on the parent (the capped cells: the cap)
LARGE_CAP = 3
FREE = (0, 4, 8)
CURVED = FREE + (1, 5, 9, 13)


def instance(ipm, shape, seed, cls, sparse_a):
    """(A, b, c, keyword arguments of IpmSolver for that class)."""
    from interiorpointmethod_amd.workloads import synthetic_lp
    m, n = shape
    A, _, c = synthetic_lp(m, n, seed)
    if sparse_a:
        keep = np.abs(A) >= 0.6
        keep[np.arange(n) % m, np.arange(n)] = True
        A = np.where(keep, A, 0.0)
    b = A @ np.ones((n, 1))
    c = np.abs(c) + 0.5
    kw = {}
    if "B" in cls:
        kw["ub"] = np.where(np.arange(n) % 4 == 3, 2.0, np.inf)
    if "Q" in cls:
        g = np.zeros(n)
        g[list(CURVED)] = 0.5 + 0.1 * np.arange(len(CURVED))
        kw["quad"] = g
    if "F" in cls:
        kw["free"] = list(FREE)
    if "D" in cls:
        kw["detect_qp" if "Q" in cls else "detect_infeasibility"] = True
    return (sparse.csc_matrix(A) if sparse_a else A), b, c, kw


def digest(sv):
    """(iterations, status, sha256) of the state the solver holds and the statistics of its last solve."""
    parts = list(sv.get_state()) + list(sv.get_bound_state() or ())
    h = hashlib.sha256()
    for a in parts:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    st = sv.stats or {}
    return dict(iterations=int(st.get("iterations", -1)), status=int(st.get("status", -1)), sha256=h.hexdigest())


def _small_kw(cls):
    return dict(quad_small="Q" in cls, free_small="F" in cls)


def _solve(sv, max_iter=200):
    sv.init_state(1.0)
    sv.solve(tol=1e-8, max_iter=max_iter)
    return digest(sv)


def cells(ipm, want=None):
    """{cell name: digest} of every cell (or of those whose path is in `want`), computed with the package `ipm`."""
    out = {}
    on = lambda path: want is None or path in want          # noqa: E731
    if on("dense"):
        for cls in CLASSES:
            A, b, c, kw = instance(ipm, SMALL_SHAPE, SEED, cls, False)
            with ipm.IpmSolver(A, b, c, **kw) as sv:
                assert not sv.schedule()["fused_small"]
                out["dense/" + cls] = _solve(sv)
    if on("small") or on("batch"):
        svs = []
        try:
            for cls in CLASSES:
                A, b, c, kw = instance(ipm, SMALL_SHAPE, SEED, cls, True)
                svs.append(ipm.IpmSolver(A, b, c, **dict(kw, **_small_kw(cls))))
                assert svs[-1].schedule()["fused_small"], cls
            if on("small"):
                for cls, sv in zip(CLASSES, svs):
                    out["small/" + cls] = _solve(sv)
            if on("batch"):
                for sv in svs:
                    sv.init_state(1.0)
                ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=200)
                for cls, sv in zip(CLASSES, svs):
                    out["batch/" + cls] = digest(sv)
        finally:
            for sv in svs:
                sv.close()
    if on("lockstep"):
        for cls in LOCKSTEP_CLASSES:
            svs = []
            try:
                for seed in (SEED, SEED + 1):
                    A, b, c, kw = instance(ipm, LOCKSTEP_SHAPE, seed, cls, True)
                    svs.append(ipm.IpmSolver(A, b, c, lockstep=True, lockstep_bounds="B" in cls, factor="dense", **kw))
                    svs[-1].init_state(1.0)
                ipm.solve_lockstep(svs, tol=1e-8, max_iter=200)
                for k, sv in enumerate(svs):
                    out["lockstep/%s/%d" % (cls, k)] = digest(sv)
            finally:
                for sv in svs:
                    sv.close()
    if on("large"):
        for cls in LARGE_CLASSES:
            A, b, c, kw = instance(ipm, LARGE_SHAPE, SEED, cls, False)
            with ipm.IpmSolver(A, b, c, **kw) as sv:
                out["large/" + cls] = _solve(sv, max_iter=LARGE_CAP)
    if on("start"):
        svs = []
        try:
            for cls in START_CLASSES:
                A, b, c, kw = instance(ipm, SMALL_SHAPE, SEED, cls, False)
                with ipm.IpmSolver(A, b, c, **kw) as sv:
                    sv.init_state_mehrotra()
                    out["start/dense/" + cls] = digest(sv)
                A, b, c, kw = instance(ipm, SMALL_SHAPE, SEED, cls, True)
                svs.append(ipm.IpmSolver(A, b, c, **kw))
                svs[-1].init_state_mehrotra()
                out["start/small/" + cls] = digest(svs[-1])
            for sv in svs:
                sv.init_state(1.0)
            ipm.init_small_batch_mehrotra(svs)
            for cls, sv in zip(START_CLASSES, svs):
                out["start-batch/" + cls] = digest(sv)
        finally:
            for sv in svs:
                sv.close()
    return out


def solved_cells(names):
    """The cells that must end in status 1: every one that runs a solve to its end (not the capped and not the start cells)."""
    return [k for k in names if k.split("/")[0] in ("dense", "small", "batch", "lockstep")]
