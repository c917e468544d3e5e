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


def separable_qp(m, n, seed, bounded=False, mixed=False):
    """Separable convex QP with a KNOWN optimum: min c.x + 1/2 x.diag(g) x, A x = b, 0 <= x (<= u)
    -> (A (m, n) dense, b, c, g, u (None unless bounded; +inf = no bound), x_star, y_star), vectors 1-D.

    A ~ N(0, 1).  A column is active with probability 0.75: x* ~ U(0.5, 2), s* = 0; otherwise x* = 0, s* ~ U(0.5, 2).  bounded: half
    the columns get u = x* + U(0.5, 2), and a tenth of the bounded active columns sit AT their bound: u = x*, z* ~ U(0.5, 2), s* = 0.
    g ~ U(0.1, 2); mixed: g = 0 on half of the inactive columns (only there: g > 0 on the support keeps x* unique).  y* ~ N(0, 1),
    c = A^T y* + s* - z* - g o x*, b = A x*: (x*, y*, s*, z*) satisfies the KKT conditions with strict complementarity.
    The columns strictly between their bounds must number at least 1.25 m (so n >= 2 m in practice): with fewer, A Theta A^T turns
    singular as the iterates converge -- a property of the problem, asserted here.  PCG64(seed)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    active = rng.random(n) < 0.75
    x = np.where(active, rng.uniform(0.5, 2.0, n), 0.0)
    s = np.where(active, 0.0, rng.uniform(0.5, 2.0, n))
    z = np.zeros(n)
    u = None
    between = active.copy()
    if bounded:
        u = np.full(n, np.inf)
        has_u = rng.random(n) < 0.5
        u[has_u] = x[has_u] + rng.uniform(0.5, 2.0, int(has_u.sum()))
        at = has_u & active & (rng.random(n) < 0.1)
        u[at] = x[at]
        z[at] = rng.uniform(0.5, 2.0, int(at.sum()))
        between &= ~at
    g = rng.uniform(0.1, 2.0, n)
    if mixed:
        g[~active & (rng.random(n) < 0.5)] = 0.0
    y = rng.standard_normal(m)
    if int(between.sum()) < 1.25 * m:
        raise AssertionError("separable_qp(%d, %d, seed=%d): %d columns strictly between their bounds, fewer than 1.25 m"
                             % (m, n, seed, int(between.sum())))
    c = A.T @ y + s - z - g * x
    return A, A @ x, c, g, u, x, y


def factor_qp(m, n, k, seed, bounded=False):
    """Factor-model QP with a KNOWN optimum: min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, 0 <= x (<= u)
    -> (A (m, n) dense, b, c, g, F (n, k), u (None unless bounded; +inf = no bound), x_star, y_star), vectors 1-D.

    Built as separable_qp builds its own: A ~ N(0, 1); a column is active with probability 0.75 (x* ~ U(0.5, 2), s* = 0), otherwise
    x* = 0, s* ~ U(0.5, 2); bounded: half the columns get u = x* + U(0.5, 2) and a tenth of the bounded active ones sit AT their
    bound (u = x*, z* ~ U(0.5, 2)); g ~ U(0.1, 2); F ~ N(0, 1) / sqrt(n); y* ~ N(0, 1); c = A^T y* + s* - z* - g o x* - F (F^T x*),
    b = A x*.  The same assertion: at least 1.25 m columns strictly between their bounds.  PCG64(seed)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    active = rng.random(n) < 0.75
    x = np.where(active, rng.uniform(0.5, 2.0, n), 0.0)
    s = np.where(active, 0.0, rng.uniform(0.5, 2.0, n))
    z = np.zeros(n)
    u = None
    between = active.copy()
    if bounded:
        u = np.full(n, np.inf)
        has_u = rng.random(n) < 0.5
        u[has_u] = x[has_u] + rng.uniform(0.5, 2.0, int(has_u.sum()))
        at = has_u & active & (rng.random(n) < 0.1)
        u[at] = x[at]
        z[at] = rng.uniform(0.5, 2.0, int(at.sum()))
        between &= ~at
    g = rng.uniform(0.1, 2.0, n)
    F = rng.standard_normal((n, k)) / np.sqrt(n)
    y = rng.standard_normal(m)
    if int(between.sum()) < 1.25 * m:
        raise AssertionError("factor_qp(%d, %d, %d, seed=%d): %d columns strictly between their bounds, fewer than 1.25 m"
                             % (m, n, k, seed, int(between.sum())))
    c = A.T @ y + s - z - g * x - F @ (F.T @ x)
    return A, A @ x, c, g, F, u, x, y


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


def free_lp(m, n, n_free, seed, bounded=False, dependent=False):
    """LP with free variables and a KNOWN optimum: min c.x, A x = b, x_j >= 0 (<= u_j) for j outside Phi, x_Phi free
    -> (A (m, n) dense, b, c, free (the sorted indices of Phi, int32), u (None unless bounded; +inf = no bound), x_star, y_star,
    s_star), vectors 1-D.

    A ~ N(0, 1); Phi = n_free columns drawn without replacement.  The free columns are basic: x* ~ +-U(0.5, 2) of either sign,
    s* = 0.  Of the barrier columns m - n_free are basic (x* ~ U(0.5, 2), s* = 0) and the rest are nonbasic (x* = 0,
    s* ~ U(0.5, 2)): strictly complementary, and the m basic columns of a Gaussian A are independent, so (x*, y*, s*) is the
    unique optimum.  bounded: half the barrier columns get u = x* + U(0.5, 2), and a tenth of the bounded NONBASIC ones sit AT
    their bound instead: x* = u ~ U(0.5, 2), s* = 0, z* ~ U(0.5, 2).  y* ~ N(0, 1), c = A^T y* + s* - z*, b = A x*.
    dependent=True (n_free >= 4): the last free column becomes a copy of the first and the one before it twice the second, so x*_Phi
    is not unique (the objective and A x = b still are); m - n_free + 2 barrier columns are basic then.  PCG64(seed)."""
    if not 1 <= n_free < n or m < 1:
        raise ValueError("free_lp needs m >= 1 and 1 <= n_free < n")
    if dependent and n_free < 4:
        raise ValueError("free_lp(dependent=True) needs n_free >= 4")
    n_basic = m - n_free + (2 if dependent else 0)
    if n_basic < 0 or n_basic > n - n_free:
        raise ValueError("free_lp: m - n_free basic barrier columns do not fit (m = %d, n = %d, n_free = %d)" % (m, n, n_free))
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    free = np.sort(rng.choice(n, n_free, replace=False))
    if dependent:
        A[:, free[-1]] = A[:, free[0]]
        A[:, free[-2]] = 2.0 * A[:, free[1]]
    barrier = np.setdiff1d(np.arange(n), free)
    basic = rng.choice(barrier, n_basic, replace=False)
    x = np.zeros(n)
    s = np.zeros(n)
    z = np.zeros(n)
    x[free] = rng.uniform(0.5, 2.0, n_free) * rng.choice([-1.0, 1.0], n_free)
    x[basic] = rng.uniform(0.5, 2.0, n_basic)
    nonbasic = np.setdiff1d(barrier, basic)
    s[nonbasic] = rng.uniform(0.5, 2.0, nonbasic.size)
    u = None
    if bounded:
        u = np.full(n, np.inf)
        has_u = barrier[rng.random(barrier.size) < 0.5]
        u[has_u] = x[has_u] + rng.uniform(0.5, 2.0, has_u.size)
        at = np.intersect1d(has_u, nonbasic)
        at = at[rng.random(at.size) < 0.1]
        x[at] = rng.uniform(0.5, 2.0, at.size)
        u[at] = x[at]
        s[at] = 0.0
        z[at] = rng.uniform(0.5, 2.0, at.size)
    y = rng.standard_normal(m)
    c = A.T @ y + s - z
    return A, A @ x, c, free.astype(np.int32), u, x, y, s
