"""Factor-model QPs: min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, 0 <= x (<= u), on the separable-QP iteration with free columns.

The quadratic term is diagonal plus low rank (a factor-model covariance, a least-squares term).  With t = F^T x as k extra
unrestricted variables, 1/2 t.t joins the DIAGONAL and the problem is the separable QP with free columns (4-U):

    A_ = [A 0; F^T -I]    b_ = [b; 0]    c_ = [c; 0]    g_ = [g; 1]    u_ = [u; +inf]    free = n .. n+k-1

Its normal matrix A_ Theta_ A_^T = [A Theta A^T, A Theta F; F^T Theta A^T, F^T Theta F + I] is symmetric positive definite of order
m + k and free of cancellation (a Sherman-Morrison downdate of A Theta A^T would lose every digit near the optimum); the dense fused
launch, the envelope factor and the sparse multifrontal factor serve it unchanged.  factor_qp_form is host arithmetic only.
A soft row or a least-squares term 1/2 ||R x - d||^2 (NNLS, constrained regression) is the same machinery with rows [R -I],
right-hand side d: factor_qp_form(A, b, c, g, R.T) and then b_[m:] = d.
With m + k <= 128 and a sparse A the augmented problem is in the class of the one-workgroup small path: free_small=True keeps it
there, and solve_small_factor_qp_batch solves a list of such problems (a risk-aversion sweep, return scenarios) in one call."""
import numpy as np

from .analysis import FUSED_SMALL_MAX_ROWS, _is_sparse, _upper_bounds
from .api import _solve_info, solve_with_info
from .batches import SMALL_TERM_LIMIT, small_batch_eligible, solve_small_batch_solvers
from .handle import SCALE_PASSES, IpmSolver, check_quadratic, check_scale


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


def factor_qp_solution(xa, ya, sa, info, F, c_, g_, m, n):
    """THE translation of a solve of the augmented problem back to the original one (solve_factor_qp and
    solve_small_factor_qp_batch both end here): (xa, ya, sa, info) as solve_with_info returns them for (A_, b_, c_, g_) of
    factor_qp_form -> (x (n, 1), y (m, 1), s (n, 1), info) with info["factors"] = k, info["t"] = the k free variables as solved,
    info["y_factor"] = the multipliers of the rows F^T x - t = 0, info["objective"] = c.x + 1/2 x.(g o x) + 1/2 ||F^T x||^2 of the x
    returned (the ORIGINAL problem's objective), the augmented problem's under info["objective_augmented"], and info["w"], info["z"]
    (bounded problems) cut to the n original columns.  A certificate of the augmented problem (detect_qp=True, status 5 / 6;
    info["certificate"]) is mapped to the ORIGINAL problem: kind 5 keeps y (m) and gets y_factor (k: the multipliers of the factor
    rows, 0 up to the violation), kind 6 keeps x (n) and gets t (k: the free variables, F^T x up to the violation); z and the other
    parts are cut to n / m.  verify_certificate(A, b, c, cert, ub=ub, g=g, F=F) checks it against the original data.
    F: n x k; the input record is not changed."""
    x, y, s = xa[:n], ya[:m], sa[:n]
    Fm, xv = np.asarray(F, dtype=np.float64), x.reshape(-1)
    ftx = Fm.T @ xv
    info = dict(info)
    info["factors"], info["t"], info["y_factor"] = xa.shape[0] - n, xa[n:].reshape(-1).copy(), ya[m:].reshape(-1).copy()
    info["objective_augmented"] = info["objective"]
    info["objective"] = float(c_[:n] @ xv + 0.5 * (g_[:n] * xv) @ xv + 0.5 * (ftx @ ftx))
    for key in ("w", "z"):
        if key in info:
            info[key] = info[key][:n]
    cert = info.get("certificate")
    if cert is not None:
        cert = dict(cert)
        ya_c, xa_c = np.asarray(cert["y"]).reshape(-1), np.asarray(cert["x"]).reshape(-1)
        cert["y"], cert["y_factor"] = ya_c[:m].copy(), ya_c[m:].copy()
        cert["x"], cert["t"] = xa_c[:n].copy(), xa_c[n:].copy()
        cert["z"] = np.asarray(cert["z"]).reshape(-1)[:n].copy()
        info["certificate"] = cert
    return x, y, s, info


def solve_factor_qp(A, b, c, F, g=None, ub=None, **opts):
    """min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, 0 <= x (<= ub) -> (x (n, 1), y (m, 1), s (n, 1), info): factor_qp_form, then
    solve_with_info(A_, b_, c_, ub=u_, quad=g_, free=free, **opts) -- every option of solve_with_info that a handle with free
    columns takes (tol, max_iter, refine, scale, factor, dense_cols, check_every, ...).  info is that solve's record with
    info["factors"] = k; info["t"] = the k free variables as solved (F^T x to the stop tolerance); info["y_factor"] = the multipliers
    of the rows F^T x - t = 0 (-t at the optimum); info["objective"] = c.x + 1/2 x.(g o x) + 1/2 ||F^T x||^2 of the x returned, the
    ORIGINAL problem's objective, with the augmented problem's (1/2 t.t in place of the last term, what the device's stop test
    saw) under info["objective_augmented"]; info["w"], info["z"] (bounded problems) are cut to the n original columns
    (factor_qp_solution).  free_small=True: a sparse A with m + k <= 128 keeps the one-workgroup small path
    (info["quadratic_path"] == "one-workgroup"; solve_small_factor_qp_batch solves a list of such problems in one call).
    detect_qp=True: the infeasibility tests of a quadratic problem (solve_with_info): info["status"] may be 5 / 6 and
    info["certificate"] is then the certificate of the ORIGINAL problem (factor_qp_solution: y and y_factor, or x and t)."""
    A_, b_, c_, g_, u_, free = factor_qp_form(A, b, c, g, F, ub)
    m, n = A_.shape[0] - free.shape[0], A_.shape[1] - free.shape[0]
    for name in ("quad", "free"):
        if name in opts:
            raise ValueError("%s: solve_factor_qp builds it from g and F" % name)
    xa, ya, sa, info = solve_with_info(A_, b_, c_, ub=u_, quad=g_, free=free, **opts)
    return factor_qp_solution(xa, ya, sa, info, F, c_, g_, m, n)


def _small_factor_qp_host_check(problems, ub):
    """Host part of solve_small_factor_qp_batch (no device is touched): per problem the shapes, factor_qp_form's own checks, the
    row limit of the small path on the AUGMENTED matrix (m + k) and its product list (the k rows F^T are dense: a column of the
    original problem feeds (c + k)(c + k + 1) / 2 terms) -> list of (A_ as CSC, b_, c_, g_ or None, u_ or None, free or None,
    F as n x k, m, n).  Every violation is a ValueError naming the problem's index."""
    from scipy import sparse
    problems = list(problems)
    if ub is not None and len(ub) != len(problems):
        raise ValueError("ub has %d entries, expected one per problem (%d)" % (len(ub), len(problems)))
    out = []
    for i, p in enumerate(problems):
        if len(p) != 5:
            raise ValueError("problem %d: expected (A, b, c, F, g), got %d entries" % (i, len(p)))
        A, b, c, F, g = p
        shape = A.shape if hasattr(A, "shape") else np.asarray(A).shape
        if len(shape) != 2:
            raise ValueError("problem %d: A must be 2-D" % i)
        m, n = int(shape[0]), int(shape[1])
        Fm = np.zeros((n, 0)) if F is None else np.asarray(F, dtype=np.float64)
        if Fm.ndim != 2 or Fm.shape[0] != n:
            raise ValueError("problem %d: F must be n x k with n = %d rows, not of shape %r" % (i, n, Fm.shape))
        k = int(Fm.shape[1])
        if m + k > FUSED_SMALL_MAX_ROWS:
            raise ValueError("problem %d has %d rows and %d factors: the small batch serves m + k <= %d (the augmented problem's rows)"
                             % (i, m, k, FUSED_SMALL_MAX_ROWS))
        try:
            A = sparse.csc_matrix(A, dtype=np.float64)            # dense A too: the small path serves sparse handles
            if A.nnz == 0:
                raise ValueError("A has no nonzero entry")
            u = None if ub is None else ub[i]
            if k:
                A_, b_, c_, g_, u_, free = factor_qp_form(A, b, c, g, Fm, u)
            else:                                                 # a plain separable QP or LP in the same list
                A_, b_, c_, free = A, _vec(b, m, "b"), _vec(c, n, "c"), None
                g_ = check_quadratic(g, n)
                u_ = None if u is None else np.asarray(u, dtype=np.float64).reshape(-1)
            u_ = _upper_bounds(u_, n + k)
        except ValueError as e:
            raise ValueError("problem %d: %s" % (i, e)) from e
        cnt = np.diff(A_.indptr).astype(np.int64)
        terms = int((cnt * (cnt + 1) // 2).sum())
        if terms > SMALL_TERM_LIMIT:
            raise ValueError("problem %d: the product list of the augmented A D^2 A^T has %d terms, the fused small path takes at most %d"
                             % (i, terms, SMALL_TERM_LIMIT))
        out.append((A_, b_, c_, g_, u_, free, Fm, m, n))
    return out


def solve_small_factor_qp_batch(problems, tol=1e-8, max_iter=5000, y0=1.0, device=0, tol_gap=None, ub=None, regularize=0.0, scale=None,
                                scale_passes=SCALE_PASSES):
    """Solve many small factor-model QPs at once -> list of (x, y, s, info), one per problem, each what
    solve_factor_qp(A, b, c, F, g, ub=..., free_small=True) returns for it alone (factor_qp_solution: factors, t, y_factor, the
    original objective, objective_augmented, w / z cut to n).

    problems: list of (A, b, c, F, g): min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, x >= 0 (x <= ub), with m + k <= 128 (the rows
    of the augmented problem); a dense A is converted to CSC.  g: None or n entries >= 0.  F: n x k, or None / k = 0 for a plain
    separable QP or LP in the same list (its record gets factors = 0 and empty t, y_factor).  ub: None or one entry per problem.
    Built like solve_small_qp_batch: the host check before any device is touched, one IpmSolver(quad=g_, free=free,
    free_small=True) per problem, init_state(y0), ONE ipm_solve_small_batch call (one workgroup per problem, one grid per kernel
    variant present), read-back, close.  Every problem error is a ValueError naming the problem's index: a bad shape,
    m + k > 128, a non-finite F, a negative or non-finite g, a product list of the augmented matrix beyond SMALL_TERM_LIMIT.
    There is no start parameter: Mehrotra's start is refused for free columns.
    solve_small_factor_qp_batch_detect is the same call with the infeasibility tests on."""
    return _solve_small_factor_qp_batch(problems, tol, max_iter, y0, device, tol_gap, ub, regularize, scale, scale_passes, False, None)


def solve_small_factor_qp_batch_detect(problems, tol=1e-8, max_iter=5000, y0=1.0, device=0, tol_gap=None, ub=None, regularize=0.0, scale=None,
                                       scale_passes=SCALE_PASSES, infeasibility_tol=(1e-8, 1e-8)):
    """solve_small_factor_qp_batch with the infeasibility tests on every member (the sibling that carries the option: the list of
    parameters of solve_small_factor_qp_batch is fixed): a member with a quadratic term is created with detect_qp=True, a plain LP in
    the list with detect_infeasibility=True.  A member that is infeasible or unbounded ends in status 5 / 6 after a few iterations
    instead of running to max_iter, with info["certificate"] mapped to its ORIGINAL problem (factor_qp_solution); every other member
    is, bit for bit, what solve_small_factor_qp_batch returns for it (the tests change no iterate).  One ipm_solve_small_batch call."""
    return _solve_small_factor_qp_batch(problems, tol, max_iter, y0, device, tol_gap, ub, regularize, scale, scale_passes, True, infeasibility_tol)


def _solve_small_factor_qp_batch(problems, tol, max_iter, y0, device, tol_gap, ub, regularize, scale, scale_passes, detect, infeasibility_tol):
    """The body of solve_small_factor_qp_batch and solve_small_factor_qp_batch_detect (detect: the infeasibility tests on every member)."""
    check_scale(scale)
    checked = _small_factor_qp_host_check(problems, ub)
    solvers = []
    try:
        for i, (A_, b_, c_, g_, u_, free, _, _, _) in enumerate(checked):
            kw = {}
            if detect:          # (check_quadratic's rule of a term: one positive entry)
                kw = dict(infeasibility_tol=infeasibility_tol, **(dict(detect_qp=True) if g_ is not None and np.any(g_ > 0) else dict(detect_infeasibility=True)))
            sv = IpmSolver(A_, b_, c_, device=device, regularize=regularize, ub=u_, scale=scale, scale_passes=scale_passes, quad=g_, free=free,
                           free_small=True, **kw)
            solvers.append(sv)
            if not small_batch_eligible(sv):
                raise ValueError("problem %d (%d x %d augmented) is not served by the fused small path (its product list is too large)"
                                 % (i, sv.m, sv.n))
            sv.init_state(y0)
        solve_small_batch_solvers(solvers, tol=tol, max_iter=max_iter, tol_gap=tol_gap)
        out = []
        for sv, (_, _, c_, g_, _, _, Fm, m, n) in zip(solvers, checked):
            xa, ya, sa = sv.get_state()
            out.append(factor_qp_solution(xa, ya, sa, _solve_info(sv, certificate=detect), Fm, c_, np.zeros(sv.n) if g_ is None else g_, m, n))
        return out
    finally:
        for sv in solvers:
            sv.close()
