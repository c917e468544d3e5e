"""Factor-model QPs: min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, 0 <= x (<= u), on the separable-QP iteration with free columns.

The quadratic term is diagonal plus low rank (a factor-model covariance, a least-squares term).  With t = F^T x as k extra
unrestricted variables, 1/2 t.t joins the DIAGONAL and the problem is the separable QP with free columns (4-U):

    A_ = [A 0; F^T -I]    b_ = [b; 0]    c_ = [c; 0]    g_ = [g; 1]    u_ = [u; +inf]    free = n .. n+k-1

Its normal matrix A_ Theta_ A_^T = [A Theta A^T, A Theta F; F^T Theta A^T, F^T Theta F + I] is symmetric positive definite of order
m + k and free of cancellation (a Sherman-Morrison downdate of A Theta A^T would lose every digit near the optimum); the dense fused
launch, the envelope factor and the sparse multifrontal factor serve it unchanged.  factor_qp_form is host arithmetic only.
A soft row or a least-squares term 1/2 ||R x - d||^2 (NNLS, constrained regression) is the same machinery with rows [R -I],
right-hand side d: factor_qp_form(A, b, c, g, R.T) and then b_[m:] = d."""
import numpy as np

from .analysis import _is_sparse
from .api import solve_with_info
from .handle import check_quadratic


def _vec(v, n, name):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.shape[0] != n:
        raise ValueError("%s has %d entries, expected %d" % (name, v.shape[0], n))
    if not np.all(np.isfinite(v)):
        raise ValueError("%s must be finite" % name)
    return v


def factor_qp_form(A, b, c, g, F, ub=None):
    """-> (A_, b_, c_, g_, u_, free) of the module docstring: A_ (m + k, n + k), CSC when A is sparse and an ndarray otherwise; b_, c_,
    g_, u_ fresh float64 vectors (u_ is None when ub is None); free = the int32 indices n .. n+k-1.  g: None (zeros) or n finite
    entries >= 0; F: n x k, k >= 1, finite; ub: None or n entries >= 0, +inf = none.  Every violation is a ValueError; no device
    is touched."""
    if _is_sparse(A):
        from scipy import sparse
        A = sparse.csc_matrix(A, dtype=np.float64)
    else:
        A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError("A must be a matrix, not %d-dimensional" % A.ndim)
    m, n = A.shape
    b, c = _vec(b, m, "b"), _vec(c, n, "c")
    F = np.asarray(F, dtype=np.float64)
    if F.ndim != 2 or F.shape[0] != n or F.shape[1] < 1:
        raise ValueError("F must be n x k with n = %d rows and k >= 1 columns, not of shape %r" % (n, F.shape))
    if not np.all(np.isfinite(F)):
        raise ValueError("F must be finite")
    k = F.shape[1]
    gq = check_quadratic(np.zeros(n) if g is None else g, n)
    g_ = np.concatenate([np.zeros(n) if gq is None else gq, np.ones(k)])
    u_ = None
    if ub is not None:
        u = np.asarray(ub, dtype=np.float64).reshape(-1)
        if u.shape[0] != n:
            raise ValueError("ub has %d entries, the problem has %d columns" % (u.shape[0], n))
        if np.any(np.isnan(u)) or np.any(u < 0):
            raise ValueError("ub must be >= 0 (+inf for none)")
        u_ = np.concatenate([u, np.full(k, np.inf)])
    if _is_sparse(A):
        from scipy import sparse
        A_ = sparse.bmat([[A, None], [sparse.csc_matrix(F.T), -sparse.identity(k, format="csc")]], format="csc")
    else:
        A_ = np.block([[A, np.zeros((m, k))], [F.T, -np.eye(k)]])
    return A_, np.concatenate([b, np.zeros(k)]), np.concatenate([c, np.zeros(k)]), g_, u_, np.arange(n, n + k, dtype=np.int32)


def solve_factor_qp(A, b, c, F, g=None, ub=None, **opts):
    """min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, 0 <= x (<= ub) -> (x (n, 1), y (m, 1), s (n, 1), info): factor_qp_form, then
    solve_with_info(A_, b_, c_, ub=u_, quad=g_, free=free, **opts) -- every option of solve_with_info that a handle with free
    columns takes (tol, max_iter, refine, scale, factor, dense_cols, check_every, ...).  info is that solve's record with
    info["factors"] = k; info["t"] = the k free variables as solved (F^T x to the stop tolerance); info["y_factor"] = the multipliers
    of the rows F^T x - t = 0 (-t at the optimum); info["objective"] = c.x + 1/2 x.(g o x) + 1/2 ||F^T x||^2 of the x returned, the
    ORIGINAL problem's objective, with the augmented problem's (1/2 t.t in place of the last term, what the device's stop test
    saw) under info["objective_augmented"]; info["w"], info["z"] (bounded problems) are cut to the n original columns."""
    A_, b_, c_, g_, u_, free = factor_qp_form(A, b, c, g, F, ub)
    m, n, k = A_.shape[0] - free.shape[0], A_.shape[1] - free.shape[0], free.shape[0]
    for name in ("quad", "free"):
        if name in opts:
            raise ValueError("%s: solve_factor_qp builds it from g and F" % name)
    xa, ya, sa, info = solve_with_info(A_, b_, c_, ub=u_, quad=g_, free=free, **opts)
    x, y, s = xa[:n], ya[:m], sa[:n]
    Fm, xv = np.asarray(F, dtype=np.float64), x.reshape(-1)
    ftx = Fm.T @ xv
    info = dict(info)
    info["factors"], info["t"], info["y_factor"] = k, xa[n:].reshape(-1).copy(), ya[m:].reshape(-1).copy()
    info["objective_augmented"] = info["objective"]
    info["objective"] = float(c_[:n] @ xv + 0.5 * (g_[:n] * xv) @ xv + 0.5 * (ftx @ ftx))
    for key in ("w", "z"):
        if key in info:
            info[key] = info[key][:n]
    return x, y, s, info
