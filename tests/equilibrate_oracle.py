"""NumPy restatement of the power-of-two Ruiz equilibration (csrc/equilibrate.h): frexp, integer floor division,
ldexp -- no floating-point rounding anywhere.  A is a dense array or a scipy sparse matrix (duplicates are summed first, as
ipm_set_A_csc does)."""
import numpy as np

try:
    from scipy import sparse as _sp
except ImportError:          # pragma: no cover
    _sp = None


def shift(v):
    """Exponent added to a line's factor for its maximum v: v = f 2^e, f in [0.5, 1) -> -floor(e / 2); v = 0 -> 0."""
    _, e = np.frexp(v)
    return np.where(v > 0, -(e.astype(np.int64) // 2), 0)


def _triplets(A):
    if _sp is not None and _sp.issparse(A):
        A = _sp.csc_matrix(A, dtype=np.float64)
        A.sum_duplicates()
        A = A.tocoo()
        return A.shape, A.row.astype(np.int64), A.col.astype(np.int64), A.data
    A = np.asarray(A, dtype=np.float64)
    i, j = np.nonzero(np.ones_like(A, dtype=bool))
    return A.shape, i, j, A.reshape(-1)


def maxima(A, er, ec):
    """Row and column maxima of 2^er_i |a_ij| 2^ec_j."""
    (m, n), i, j, v = _triplets(A)
    s = np.ldexp(np.abs(v), (er[i] + ec[j]).astype(np.int64))
    rmax, cmax = np.zeros(m), np.zeros(n)
    np.maximum.at(rmax, i, s)
    np.maximum.at(cmax, j, s)
    return rmax, cmax


def ruiz(A, passes):
    """-> (er, ec, changed): the exponents of R and C after at most `passes` simultaneous passes and the number of passes that
    changed a factor."""
    m, n = A.shape
    er, ec = np.zeros(m, dtype=np.int64), np.zeros(n, dtype=np.int64)
    changed = 0
    for _ in range(passes):
        rmax, cmax = maxima(A, er, ec)
        dr, dc = shift(rmax), shift(cmax)
        if not dr.any() and not dc.any():
            break
        er, ec, changed = er + dr, ec + dc, changed + 1
    return er, ec, changed


def factors(er, ec):
    return np.ldexp(1.0, er), np.ldexp(1.0, ec)


def prescale(A, b, c, u, er, ec):
    """(R A C, R b, C c, u / C) by ldexp applied entrywise; u may be None."""
    if _sp is not None and _sp.issparse(A):
        S = _sp.csc_matrix(A, dtype=np.float64)
        S.sum_duplicates()
        S = S.tocoo()
        A2 = _sp.csc_matrix((np.ldexp(S.data, er[S.row] + ec[S.col]), (S.row, S.col)), shape=S.shape)
    else:
        A = np.asarray(A, dtype=np.float64)
        A2 = np.ldexp(A, er[:, None] + ec[None, :])
    b2 = np.ldexp(np.asarray(b, dtype=np.float64).reshape(-1), er)
    c2 = np.ldexp(np.asarray(c, dtype=np.float64).reshape(-1), ec)
    u2 = None if u is None else np.ldexp(np.asarray(u, dtype=np.float64).reshape(-1), -ec)
    return A2, b2, c2, u2
