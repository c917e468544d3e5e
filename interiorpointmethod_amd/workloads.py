"""Benchmark workloads of BASELINE.json (inputs only; no solver code)."""
from __future__ import annotations

import numpy as np


def synthetic_lp(m, n, seed=0):
    """Strictly primal-dual feasible dense LP of SURVEY.md 8(d).

    PCG64 draws in this order: A ~ N(0,1) (m,n); x0 ~ U(0.5,1.5) (n,1); y0 ~ N(0,1) (m,1);
    s0 ~ U(0.5,1.5) (n,1); b = A x0; c = A^T y0 + s0.  Pin: A[0,0] = 0.1257302210933933.
    """
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    x0 = rng.uniform(0.5, 1.5, (n, 1))
    y0 = rng.standard_normal((m, 1))
    s0 = rng.uniform(0.5, 1.5, (n, 1))
    return A, A @ x0, A.T @ y0 + s0


def flops_per_iteration(m, n, nnz_col_sq=None):
    """Algorithmic flops of one iteration: m^2 n + m^3/3 + 4 m^2 + 12 m n;
    for a sparse A the contraction term is sum_j nnz(A[:,j])^2."""
    form = float(m) * m * n if nnz_col_sq is None else float(nnz_col_sq)
    return form + m ** 3 / 3.0 + 4.0 * m * m + 12.0 * m * n


def block_angular_lp(m, block, k, seed=0, link_fill=0.5):
    """Block-angular LP with k linking columns: A = [block-diagonal sparse part | k linking columns | identity], m rows
    in blocks of `block` consecutive rows -> (A as scipy CSC, b (m, 1), c (n, 1), the indices of the linking columns).

    Block part, per block: a chain (one column over each pair of consecutive rows) and as many columns over three random rows of
    the block -- A A^T of it is block diagonal with an elimination tree as deep as the block.  A linking column has a N(0, 1) entry
    in each row with probability link_fill (at least one per block), so A A^T as a whole is full.  The identity keeps every row
    non-empty without the linking columns and A of full row rank.  Strictly primal-dual feasible, hence feasible and bounded, by
    construction: x0, s0 ~ U(0.5, 1.5), y0 ~ N(0, 1), b = A x0, c = A^T y0 + s0 (as synthetic_lp).  PCG64(seed)."""
    from scipy import sparse as sp
    if m < 2 or block < 2 or k < 0:
        raise ValueError("block_angular_lp needs m >= 2, block >= 2, k >= 0")
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    ncol = 0
    for r0 in range(0, m, block):
        r1 = min(m, r0 + block)
        for i in range(r0, r1 - 1):                                   # the chain
            rows += [i, i + 1]; cols += [ncol, ncol]; vals += list(rng.standard_normal(2)); ncol += 1
        if r1 - r0 >= 3:
            for _ in range(r1 - r0):                                  # three random rows of the block
                rows += list(rng.choice(np.arange(r0, r1), 3, replace=False)); cols += [ncol] * 3; vals += list(rng.standard_normal(3)); ncol += 1
    link = np.arange(ncol, ncol + k)
    for j in link:
        hit = rng.random(m) < link_fill
        for r0 in range(0, m, block):
            if not hit[r0:r0 + block].any():
                hit[r0] = True
        idx = np.flatnonzero(hit)
        rows += list(idx); cols += [j] * idx.size; vals += list(rng.standard_normal(idx.size))
    ncol += k
    rows += list(range(m)); cols += list(range(ncol, ncol + m)); vals += [1.0] * m
    n = ncol + m
    A = sp.csc_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=(m, n))
    A.sum_duplicates(); A.sort_indices()
    x0 = rng.uniform(0.5, 1.5, (n, 1))
    y0 = rng.standard_normal((m, 1))
    s0 = rng.uniform(0.5, 1.5, (n, 1))
    return A, A @ x0, A.T @ y0 + s0, link
