"""Infeasible and unbounded LPs with known certificates (host only): the instances of the infeasibility tests
(IPM_FLAG_DETECT_INFEASIBILITY).  Every instance is confirmed by scipy's HiGHS in
tests/test_infeasibility_host.py and solved on the device in tests/test_gpu_infeasibility.py.

Each builder returns a dict: A (dense ndarray or scipy CSC), b, c (1-D), ub (None or length n, +inf = none), kind
("primal_infeasible" / "dual_infeasible") and, where the construction gives one, the exact certificate `cert`."""
import os

import numpy as np
from scipy import sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netlib")
KIND = {"primal_infeasible": 5, "dual_infeasible": 6}


def netlib(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    m, n = (int(v) for v in d["shape"])
    A = sparse.csc_matrix((d["data"], d["indices"], d["indptr"]), shape=(m, n))
    return A, np.asarray(d["b"], dtype=np.float64).reshape(-1), np.asarray(d["c"], dtype=np.float64).reshape(-1)


def primal_infeasible_dense(m=40, n=90, seed=0):
    """Construction 1: A^T y* <= -r < 0 and b.y* = 1, c > 0."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    ys = rng.standard_normal(m)
    A -= np.outer(ys, np.maximum(A.T @ ys, 0.0) + rng.random(n)) / (ys @ ys)
    b = rng.standard_normal(m)
    b += (1.0 - b @ ys) * ys / (ys @ ys)
    c = rng.random(n) + 0.1
    return dict(A=A, b=b, c=c, ub=None, kind="primal_infeasible", cert=dict(kind="primal_infeasible", y=ys, z=np.zeros(n)))


def dual_infeasible_dense(m=40, n=90, seed=0, density=1.0):
    """Construction 2: A d = 0 with d > 0, b = A x0 with x0 > 0, c.d = -1.  density < 1: that share of the entries of A (but
    the last column) nonzero -- still a dense array."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    if density < 1.0:
        A *= rng.random((m, n)) < density
    d = rng.random(n) + 0.5
    A[:, -1] = -(A[:, :-1] @ d[:-1]) / d[-1]
    x0 = rng.random(n) + 0.5
    b = A @ x0
    c = rng.standard_normal(n)
    c -= (c @ d + 1.0) * d / (d @ d)
    return dict(A=A, b=b, c=c, ub=None, kind="dual_infeasible", cert=dict(kind="dual_infeasible", x=d), x0=x0)


def afiro_duplicate_row():
    """3(a): AFIRO with row 3 duplicated, right-hand side b_3 + 1."""
    A, b, c = netlib("AFIRO")
    A2 = sparse.vstack([A, A[3]], format="csc")
    y = np.zeros(A.shape[0] + 1); y[-1] = 1.0; y[3] = -1.0
    return dict(A=A2, b=np.append(b, b[3] + 1.0), c=c, ub=None, kind="primal_infeasible",
                cert=dict(kind="primal_infeasible", y=y, z=np.zeros(A.shape[1])))


def add_negative_sum_row(A, b, c):
    """3(b): an added row sum(x) = -1 (certificate y = -e_new)."""
    m, n = A.shape
    A2 = sparse.vstack([sparse.csc_matrix(A), sparse.csc_matrix(np.ones((1, n)))], format="csc")
    y = np.zeros(m + 1); y[-1] = -1.0
    return dict(A=A2, b=np.append(b, -1.0), c=c, ub=None, kind="primal_infeasible", cert=dict(kind="primal_infeasible", y=y, z=np.zeros(n)))


def add_free_ray_column(A, b, c):
    """3(c): an added zero column with cost -1 (ray e_new)."""
    m, n = A.shape
    A2 = sparse.hstack([sparse.csc_matrix(A), sparse.csc_matrix((m, 1))], format="csc")
    x = np.zeros(n + 1); x[-1] = 1.0
    return dict(A=A2, b=b, c=np.append(c, -1.0), ub=None, kind="dual_infeasible", cert=dict(kind="dual_infeasible", x=x))


def afiro_negative_sum_row():
    return add_negative_sum_row(*netlib("AFIRO"))


def afiro_free_ray_column():
    return add_free_ray_column(*netlib("AFIRO"))


def bounded_primal_infeasible(m=40, n=90, k=10, seed=1):
    """4: feasible without the bounds, infeasible with them: a row sum_{j in S} x_j = |S| + 1 and u_S = 1 (certificate
    y = e_new, z_S = 1: it needs z)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    x0 = rng.random(n) + 0.5
    S = np.arange(k)
    x0[S] = 1.0 + 1.0 / k
    row = np.zeros(n); row[S] = 1.0
    A = np.vstack([A, row])
    b = A @ x0
    ub = np.full(n, np.inf); ub[S] = 1.0
    ub[k:2 * k] = 3.0                                     # (more bounded columns that the certificate does not need)
    y = np.zeros(m + 1); y[-1] = 1.0
    z = np.zeros(n); z[S] = 1.0
    return dict(A=A, b=b, c=rng.random(n) + 0.1, ub=ub, kind="primal_infeasible", cert=dict(kind="primal_infeasible", y=y, z=z))


def bounded_dual_infeasible(m=40, n=90, k=10, seed=2):
    """4: unbounded with bounds on U = the first k columns, along a ray d that avoids U (d_U = 0)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    d = rng.random(n) + 0.5
    d[:k] = 0.0
    A[:, -1] = -(A[:, :-1] @ d[:-1]) / d[-1]
    x0 = rng.random(n) + 0.5
    x0[:k] = 0.5
    b = A @ x0
    ub = np.full(n, np.inf); ub[:k] = 1.0
    c = rng.standard_normal(n)
    c -= (c @ d + 1.0) * d / (d @ d)
    return dict(A=A, b=b, c=c, ub=ub, kind="dual_infeasible", cert=dict(kind="dual_infeasible", x=d))


# 5: mid-size sparse Netlib instances (m > 128) with the 3(b) / 3(c) edits
MID_NETLIB = ("SC205", "SCTAP1", "E226")


def netlib_negative_sum_row(name):
    return add_negative_sum_row(*netlib(name))


def netlib_free_ray_column(name):
    return add_free_ray_column(*netlib(name))


def large_dense(seed=3):
    """6: 21 blocks of 128 rows (2688 x 5376), construction 2: the fused formation + factorization launch runs.  (Too large for
    HiGHS within a test's time: tests/test_infeasibility_host.py proves it unbounded from its feasible point x0 and its ray.)"""
    return dual_infeasible_dense(21 * 128, 42 * 128, seed=seed, density=0.02)


def small_instances():
    """Every instance small enough for the NumPy oracle (name -> builder)."""
    return {
        "primal_dense": primal_infeasible_dense,
        "dual_dense": dual_infeasible_dense,
        "afiro_dup_row": afiro_duplicate_row,
        "afiro_neg_row": afiro_negative_sum_row,
        "afiro_ray_col": afiro_free_ray_column,
        "bounded_primal": bounded_primal_infeasible,
        "bounded_dual": bounded_dual_infeasible,
    }


def mid_instances():
    out = {}
    for nm in MID_NETLIB:
        out[nm + "_neg_row"] = (lambda nm=nm: netlib_negative_sum_row(nm))
        out[nm + "_ray_col"] = (lambda nm=nm: netlib_free_ray_column(nm))
    return out


def all_instances(large=True):
    d = dict(small_instances())
    d.update(mid_instances())
    if large:
        d["large_dense"] = large_dense
    return d


def oracle_detection(A, b, c, eps=1e-8, max_iter=200, y0=1.0):
    """First iteration k at which the NumPy oracle's iterate (no bounds) passes a test of DESIGN.md 4-C -> (k, kind) or
    (None, status string) when the loop ends first."""
    from oracle import ipm_oracle as O
    A, b, c = O.as_float64_problem(A, b, c)
    m, n = A.shape
    x, y, s = O.initial_point(m, n, y0)
    for k in range(max_iter + 1):
        if not O.check_optimality(A, b, c, x, y, s, 1e-8, 1e-8, 1e-8):
            return None, "converged"
        aty = np.asarray(A.T @ y).reshape(-1)
        beta = float(b.T @ y)
        if beta > 0 and np.max(np.maximum(aty, 0.0)) <= eps * beta:
            return k, "primal_infeasible"
        gamma = -float(c.T @ x)
        if gamma > 0 and np.max(np.abs(np.asarray(A @ x))) <= eps * gamma:
            return k, "dual_infeasible"
        x, y, s, _ = O.iterate(A, b, c, x, y, s)
        if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(s))):
            return None, "nan"
    return None, "max_iter"
