"""Cases and oracles of the dense-column split of the sparse factor (host only).

arrowhead(): A = [block-diagonal sparse part | k dense columns | identity].  split_oracle(): the five formulas of the split restated
in NumPy float64.  longdouble_solve(): a direct Cholesky solve of the FULL B = A diag(d) A^T in np.longdouble, the reference both
the oracle and the device are measured against."""
import os

import numpy as np
from scipy import sparse
from scipy.linalg import cholesky, solve_triangular

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netlib")
EPS = np.finfo(np.float64).eps


def netlib(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    m, n = (int(v) for v in d["shape"])
    A = sparse.csc_matrix((d["data"], d["indices"], d["indptr"]), shape=(m, n))
    return A, np.asarray(d["b"], dtype=np.float64).reshape(-1), np.asarray(d["c"], dtype=np.float64).reshape(-1)


def arrowhead(m=300, k=17, block=50, seed=0):
    """-> (A as canonical CSC, the indices of the k dense columns).  Block part: per block of `block` consecutive rows a chain (a
    column over each pair of consecutive rows) and as many columns over three random rows of the block: the elimination tree of
    its normal matrix is at least three panel levels deep (tests/test_dense_split_host.py checks it).  Dense column 0 touches
    EVERY row, dense column 1 only the rows of the first block (a single leaf block), the others a random half of the rows.  The
    identity keeps every row non-empty without the dense columns."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    ncol = 0
    for r0 in range(0, m, block):
        r1 = min(m, r0 + block)
        for i in range(r0, r1 - 1):
            rows += [i, i + 1]; cols += [ncol, ncol]; vals += list(rng.standard_normal(2)); ncol += 1
        if r1 - r0 >= 3:
            for _ in range(r1 - r0):
                rows += list(rng.choice(np.arange(r0, r1), 3, replace=False)); cols += [ncol] * 3; vals += list(rng.standard_normal(3)); ncol += 1
    dense = np.arange(ncol, ncol + k, dtype=np.int32)
    for t, j in enumerate(dense):
        if t == 0:
            idx = np.arange(m)
        elif t == 1:
            idx = np.arange(min(block, m))
        else:
            idx = np.flatnonzero(rng.random(m) < 0.5)
        rows += list(idx); cols += [j] * idx.size; vals += list(rng.standard_normal(idx.size))
    ncol += k
    rows += list(range(m)); cols += list(range(ncol, ncol + m)); vals += [1.0] * m
    A = sparse.csc_matrix((np.asarray(vals), (np.asarray(rows), np.asarray(cols))), shape=(m, ncol + m))
    A.sum_duplicates(); A.sort_indices()
    return A, dense


def spread_d(n, decades, seed=0):
    """d with log10 uniform over [-decades, +decades] (decades = 0: all ones)."""
    if decades == 0:
        return np.ones(n)
    return 10.0 ** np.random.default_rng(seed).uniform(-decades, decades, n)


def split_parts(A, cols, d):
    """(A_s D_s A_s^T dense, V) in float64: the matrix the sparse factor holds and V = A_DC diag(sqrt(d_DC))."""
    A = sparse.csc_matrix(A)
    keep = np.ones(A.shape[1], dtype=bool)
    keep[cols] = False
    As = A[:, keep]
    Bs = (As @ sparse.diags(d[keep]) @ As.T).toarray()
    V = A[:, cols].toarray() * np.sqrt(d[cols])[None, :]
    return Bs, V


def split_oracle(A, cols, d, t):
    """The split's formulas in NumPy float64 -> dict(dy, L, V, W, S, R, z0, Bs):  B_s = L L^T, V, W = L^-1 V, S = I + W^T W = R R^T,
    z = L^-1 t, z -= W (S^-1 (W^T z)), dy = L^-T z."""
    Bs, V = split_parts(A, cols, d)
    L = cholesky(Bs, lower=True)
    W = solve_triangular(L, V, lower=True)
    S = np.eye(len(cols)) + W.T @ W
    R = cholesky(S, lower=True)
    z0 = solve_triangular(L, t, lower=True)
    u = W.T @ z0
    v = solve_triangular(R, solve_triangular(R, u, lower=True), lower=True, trans="T")
    z = z0 - W @ v
    dy = solve_triangular(L, z, lower=True, trans="T")
    return dict(dy=dy, L=L, V=V, W=W, S=S, R=R, z0=z0, Bs=Bs)


def longdouble_solve(A, d, t):
    """B^-1 t with B = A diag(d) A^T, everything in np.longdouble: formation, a column Cholesky without pivoting, both sweeps."""
    Ad = np.asarray(sparse.csc_matrix(A).toarray(), dtype=np.longdouble)
    B = (Ad * np.asarray(d, dtype=np.longdouble)[None, :]) @ Ad.T
    m = B.shape[0]
    L = np.zeros_like(B)
    for j in range(m):
        col = B[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = col / np.sqrt(col[0])
    z = np.asarray(t, dtype=np.longdouble).copy()
    for j in range(m):
        z[j] = (z[j] - L[j, :j] @ z[:j]) / L[j, j]
    for j in range(m - 1, -1, -1):
        z[j] = (z[j] - L[j + 1:, j] @ z[j + 1:]) / L[j, j]
    return z


def fit1p_reference():
    """(t, B^-1 t in np.longdouble) for FIT1P's full B = A A^T (d = 1): longdouble_solve(A, 1, t) with t = the standard normal
    draws of PCG64(4), recorded once in tests/golden/dense_split_fit1p_ref.npz as a float64 pair hi + lo (the column Cholesky
    of 1026 rows in np.longdouble takes most of a minute on the host)."""
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "dense_split_fit1p_ref.npz"))
    return g["t"], g["hi"].astype(np.longdouble) + g["lo"].astype(np.longdouble)


def rel_err(x, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.linalg.norm(np.asarray(x, dtype=np.longdouble) - ref) / np.linalg.norm(ref))


def oracle_bound(A, cols, d, t, ref):
    """Bound on the oracle's forward error against the direct solve, derived, not picked: every pair of sweeps with L solves with
    B_s to a relative error of gamma cond_2(B_s) (Higham, Accuracy and Stability, thm 10.4 with 8.5), gamma = 4 m eps for the four
    sweep-sized steps of the split (L^-1 t, W, the k x k solve inside cond(S) <= cond(B_s), L^-T z); that error is relative to
    the UNCORRECTED solution y0 = B_s^-1 t, from which the correction subtracts, so it is amplified by ||y0|| / ||dy|| >= 1 when
    read against dy.  -> (bound, cond_2(B_s), amplification)."""
    Bs, _ = split_parts(A, cols, d)
    cond = float(np.linalg.cond(Bs))
    y0 = np.linalg.solve(Bs, t)
    amp = max(1.0, float(np.linalg.norm(y0) / np.linalg.norm(np.asarray(ref, dtype=np.float64))))
    m = Bs.shape[0]
    return 4.0 * m * EPS * cond * amp, cond, amp
