"""The direction and linear-solve seams of the reference's call surface, and the unreduced KKT system on the device LU:

    direction_predicted_sparse(..., method="normal"|"full") -> (dx, dy, ds)   main.py:197-229
    direction_corrected_sparse(...)     -> (dx, dy, ds)              main.py:247-269
    direction_predicted / direction_corrected (dense-path names)     main.py:185-194, 232-244
    solve_linear(B, rhs)                -> (N, 1)                    main.py:176-182"""
import ctypes as C

import numpy as np

from . import _lib
from .analysis import _col, _is_sparse, _sp
from .handle import IpmSolver, _dptr

_METHODS = ("normal", "full", "kkt")


def _dense(M):
    return np.asarray(M.toarray() if _is_sparse(M) else M, dtype=np.float64)


def _kkt_matrix(A, x, s):
    """The reference's unreduced Newton matrix [[0, A^T, I], [A, 0, 0], [S, 0, X]] of order 2n + m (main.py:13-21,
    create_sparse_matrix sparse_interior.py:12), dense, assembled by scattering the nonzeros of A (duplicates summed)."""
    m, n = A.shape
    N = 2 * n + m
    K = np.zeros((N, N))
    if _is_sparse(A):
        Ac = _sp.coo_matrix(_sp.csr_matrix(A, dtype=np.float64))       # csr: duplicates summed, as scipy does
        i, j, v = Ac.row, Ac.col, Ac.data
    else:
        Ad = np.asarray(A, dtype=np.float64)
        i, j = np.nonzero(Ad)
        v = Ad[i, j]
    K[n + i, j] = v                        # A
    K[j, n + i] = v                        # A^T
    d = np.arange(n)
    K[d, n + m + d] = 1.0                  # I
    K[n + m + d, d] = np.asarray(s, dtype=np.float64).ravel()    # S
    K[n + m + d, n + m + d] = np.asarray(x, dtype=np.float64).ravel()   # X
    return K


def _kkt_residuals(A, b, c, x, y, s):
    m, n = A.shape
    x, y, s = _col(x, n, "x"), _col(y, m, "y"), _col(s, n, "s")
    bb, cc = _col(b, m, "b"), _col(c, n, "c")
    At = A.T
    rb = np.asarray(A @ x).ravel() - bb              # main.py:84-88
    rc = np.asarray(At @ y).ravel() + s - cc
    return x, y, s, rb, rc


def _kkt_solve(A, x, s, rc, rb, r3, device):
    m, n = A.shape
    K = _kkt_matrix(A, x, s)
    sol = lu_solve(K, np.concatenate([-rc, -rb, -r3]), device=device)
    return sol[:n].reshape(-1, 1), sol[n:n + m].reshape(-1, 1), sol[n + m:].reshape(-1, 1)


def _ratio(v, dv):
    neg = dv < 0
    return float(min(1.0, np.min(-v[neg] / dv[neg]))) if neg.any() else 1.0


def _kkt_predicted(A, b, c, x, y, s, device):
    """method="kkt" of the predictor: the reference's method="full" (main.py:198-212) -- the unreduced system with
    right-hand side [-(A^T y + s - c); -(A x - b); -x s] (create_rhs_predicted, main.py:79-108) by the device LU."""
    x, y, s, rb, rc = _kkt_residuals(A, b, c, x, y, s)
    return _kkt_solve(A, x, s, rc, rb, x * s, device)


def _kkt_corrected(A, b, c, x, y, s, dxa, dya, dsa, device):
    """method="kkt" of the corrector (main.py:247-265): the GIVEN affine direction enters through the centering
    sigma = (mu_aff / mu)^3 (duality_gap, main.py:588-601) and r4 = x s + dx_aff ds_aff - sigma mu (main.py:150-158)."""
    if dxa is None or dya is None or dsa is None:
        raise ValueError('method="kkt" needs delta_x_aff, delta_y_aff and delta_s_aff (the corrector uses them as given)')
    m, n = A.shape
    x, y, s, rb, rc = _kkt_residuals(A, b, c, x, y, s)
    dxa, dsa = _col(dxa, n, "delta_x_aff"), _col(dsa, n, "delta_s_aff")
    ap, ad = _ratio(x, dxa), _ratio(s, dsa)                      # predicted_stepsize, main.py:305-322
    mu_aff = float(np.dot(x + ap * dxa, s + ad * dsa)) / n
    mu = float(np.dot(x, s)) / n
    sigma = (mu_aff / mu) ** 3
    r4 = x * s + dxa * dsa - sigma * mu
    return _kkt_solve(A, x, s, rc, rb, r4, device)


def direction_predicted_sparse(A, b, c, x, y, s, method="normal", device=0):
    """main.py:197: predictor direction at (x, y, s).  method="normal" (main.py:221-229) and method="full" (the
    unreduced KKT system of main.py:198-212) define the same direction; the device solves both through the normal
    equations (the Schur complement of the full system), which agrees with the reference's method="full" LU to 1e-11
    at a well-conditioned point (tests/test_gpu_parity.py::test_direction_kats).  method="kkt" solves the reference's
    unreduced (2n + m)-order system itself with the device LU (lu_solve): the reference's method="full" arithmetic,
    also late in a solve where the two formulations drift apart."""
    if method not in _METHODS:
        raise ValueError('method must be "normal", "full" or "kkt" (the "eliminate" variant of the reference uses a wrong '
                         'right-hand side, main.py:270-276, and is not mirrored)')
    if method == "kkt":
        return _kkt_predicted(A, b, c, x, y, s, device)
    with IpmSolver(A, b, c, device=device) as sv:
        sv.set_state(x, y, s)
        return sv.newton_direction(corrector=False)


def direction_corrected_sparse(A, b, c, x, y, s, delta_x_aff=None, delta_y_aff=None, delta_s_aff=None,
                               method="full", device=0):
    """main.py:247: corrector direction (the reference's default method here is "full").  With "normal" / "full" the
    affine direction is recomputed on the device from (x, y, s) (same factor reused), so the delta_*_aff arguments are
    accepted for signature compatibility only; method="kkt" uses the delta_*_aff given (required) and solves the
    unreduced system with the device LU, as the reference's method="full" does."""
    if method not in _METHODS:
        raise ValueError('method must be "normal", "full" or "kkt"')
    if method == "kkt":
        return _kkt_corrected(A, b, c, x, y, s, delta_x_aff, delta_y_aff, delta_s_aff, device)
    with IpmSolver(A, b, c, device=device) as sv:
        sv.set_state(x, y, s)
        sv.newton_direction(corrector=False)
        return sv.newton_direction(corrector=True)


def direction_predicted(A, b, c, x, y, s, device=0, method="full"):
    """Dense-path name of the same seam (main.py:185-194); method="kkt": the reference's own unreduced system by LU."""
    return direction_predicted_sparse(np.asarray(A, dtype=np.float64), b, c, x, y, s, method=method, device=device)


def direction_corrected(A, b, c, x, y, s, delta_x_aff=None, delta_y_aff=None, delta_s_aff=None, device=0, method="full"):
    """Dense-path name of the corrector seam (main.py:232-244); method="kkt" as in direction_corrected_sparse."""
    return direction_corrected_sparse(np.asarray(A, dtype=np.float64), b, c, x, y, s, delta_x_aff, delta_y_aff,
                                      delta_s_aff, method=method, device=device)


def _square(A):
    M = np.ascontiguousarray(_dense(A))
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 1:
        raise ValueError("A must be a non-empty square matrix, got shape %s" % (M.shape,))
    return M


def _lu_error(code, who):
    msg = (_lib.load().ipm_last_error(None) or b"").decode("utf-8", "replace")
    if code == _lib.ERR_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix (%s: %s)" % (who, msg))
    raise _lib.IpmError(code, msg)


def lu_solve(A, b, device=0):
    """A x = b for a general square A by LU with partial pivoting on the GPU (ipm_lu_solve): what the reference's
    np.linalg.solve does (main.py:178).  b of shape (n,), (n, 1) or (n, k); the result has the shape of b.  A singular A
    raises numpy.linalg.LinAlgError, as np.linalg.solve does."""
    M = _square(A)
    n = M.shape[0]
    rhs = np.asarray(b, dtype=np.float64)
    if rhs.shape[0] != n or rhs.ndim not in (1, 2):
        raise ValueError("b must have shape (%d,), (%d, 1) or (%d, k), got %s" % (n, n, n, rhs.shape))
    B = np.ascontiguousarray(rhs.reshape(n, -1))
    k = B.shape[1]
    X = np.empty_like(B)
    info = C.c_int64(0)
    code = _lib.load().ipm_lu_solve(int(device), n, _dptr(M), n, k, _dptr(B), k, _dptr(X), k, C.byref(info))
    if code != _lib.IPM_OK:
        _lu_error(code, "ipm_lu_solve")
    return X.reshape(rhs.shape)


def lu_factor(A, device=0):
    """(LU, piv) of P A = L U on the GPU (ipm_lu_factor), in scipy.linalg.lu_factor's convention: unit L below the
    diagonal and U on and above it packed in LU, row i interchanged with row piv[i] (0-based, in order).  An exactly
    zero pivot does not stop the factorization; it is reported with a warning, as scipy does."""
    M = _square(A)
    n = M.shape[0]
    LU = np.empty_like(M)
    piv = np.empty(n, dtype=np.int32)
    info = C.c_int64(0)
    code = _lib.load().ipm_lu_factor(int(device), n, _dptr(M), n, _dptr(LU), n,
                                     piv.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info))
    if code == _lib.ERR_SINGULAR:
        import warnings
        warnings.warn("Diagonal number %d is exactly zero. Singular matrix." % info.value, RuntimeWarning, stacklevel=2)
    elif code != _lib.IPM_OK:
        _lu_error(code, "ipm_lu_factor")
    return LU, piv


def solve_linear(A, b, method="hip", device=0):
    """main.py:176-182.  method="lu": any square A by LU with partial pivoting on the GPU (the reference's default,
    np.linalg.solve; see lu_solve), result in the shape of b.  Any other method (the default "hip"): A symmetric positive
    (semi)definite, guarded Cholesky on the GPU (only the lower triangle is read), result (n, 1)."""
    if method == "lu":
        return lu_solve(A, b, device=device)
    B = np.asarray(A.todense() if _is_sparse(A) else A, dtype=np.float64)
    m = B.shape[0]
    rhs = np.asarray(b, dtype=np.float64).reshape(-1)
    with IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1), device=device) as sv:
        z, _ = sv.solve_linear(B, rhs)
    return z
