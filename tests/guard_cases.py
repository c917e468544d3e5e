"""Normal matrices whose pivot-guard decisions are exact (test_guard_cases.py checks the construction on the host,
test_gpu_pivot_guard.py runs it through every dense Cholesky path).

B = A diag(d) A^T with A = [L0 | zero columns] and L0 = D + N:
  - D is diagonal, 1 on every row except the GUARDED ones (0 there);
  - N is strictly lower triangular with entries +-1.  Its nonzero columns are HUB rows, its nonzero rows are the
    COUPLED rows (unguarded) and the DEPENDENT rows (guarded); hubs are never coupled or dependent, so N N = 0.  Every
    hub serves exactly one row, so two rows never share a hub: the Schur complement of a guarded column is exactly zero
    and no product of a guarded column's 1/sqrt(big) with a nonzero ever reaches an unguarded column.
  - A dependent row is an exact combination of its hub rows; an EMPTY row (row 0 always) has no entries at all.
  - DECOUPLED rows are plain identity rows whose diagonal d_j is chosen (x_j / s_j with s_j = 1 on the LP paths): one of
    them sets max diag(B) to `maxdiag`, the optional boundary rows sit exactly at eps * maxdiag and one ulp on either side,
    and an optional row holds -1 (guarded; it cannot raise the max).

Every intermediate value of the factorization is then a small integer (or the chosen power of two), so with unit pivots
the unguarded columns of L are those of L0 bitwise, a guarded pivot is exactly 0.0 whatever the summation order, and the
guarded factor is L0 with each guarded column replaced by sqrt(big) e_j."""
import numpy as np

BIG = 1e64
EPS = 1e-30


def guard_rows(m):
    """The guarded rows for order m, placed where the kernels change regime: row 0, the 16-wide tile edges 15/16, the
    128-row block edges 127/128, the last true row, a full 16-row panel, a full 128-row block (m >= 512), a row in the
    last whole 1024-row group (m >= 2048).  m = 1: none (the one row carries the max of the diagonal)."""
    if m < 2:
        return []
    rows = {0, 15, 16, 127, 128, m - 1}
    if m >= 300:
        rows |= set(range(240, 256))                   # panel 15 of block 1: the last panel of a block
    elif m >= 64:
        rows |= set(range(32, 48))
    if m >= 512:
        rows |= set(range(256, 384))                   # all of block 2
    if m >= 2048:
        rows |= {1024 * (m // 1024) - 48}              # inside the last whole group of the grouped inverses
    return sorted(r for r in rows if 0 <= r < m)


class GuardCase:
    """One exact case.  Attributes: m, n, L0 (m x m), A (m x n dense), d (n,), guarded (sorted row indices),
    empty (rows with no entries), decoupled (dict row -> diagonal), maxdiag, eps."""

    def __init__(self, m, guarded=None, seed=0, maxdiag=64.0, eps=EPS, boundary=False, negative=False,
                 coupled_frac=0.25, n_extra=8, empty=None):
        rng = np.random.default_rng(seed + 1000 * m)
        self.m, self.eps, self.maxdiag = m, eps, float(maxdiag)
        G = sorted(set(guard_rows(m) if guarded is None else guarded))
        used = set(G)
        free = lambda: [r for r in range(m) if r not in used]            # noqa: E731
        # decoupled rows: the max of the diagonal, then the threshold rows and the -1 row (all guarded but t+)
        self.decoupled = {}
        t = eps * self.maxdiag                        # the library's own product: eps * max diag(B)
        special = [("max", self.maxdiag)]
        if boundary:
            special += [("t-", np.nextafter(t, 0.0)), ("t", t), ("t+", np.nextafter(t, np.inf))]
        if negative:
            special += [("neg", -1.0)]
        self.role = {}
        cand = free()
        if len(cand) < len(special):
            raise ValueError("m = %d is too small for %d decoupled rows" % (m, len(special)))
        picks = rng.choice(cand, size=len(special), replace=False)
        for (name, v), r in zip(special, sorted(int(p) for p in picks)):
            self.decoupled[r] = float(v)
            self.role[name] = r
            used.add(r)
        # dependent rows get 1-2 private hubs, as early as possible (earlier blocks / groups); empty rows get none
        self.empty = sorted(set([0] if 0 in G else []) | set(e for e in (empty or []) if e in G))
        N = np.zeros((m, m))
        for j in G:
            if j in self.empty:
                continue
            hubs = [h for h in free() if h < j]
            if not hubs:
                self.empty.append(j)
                continue
            k = min(len(hubs), 1 + int(rng.integers(0, 2)))
            # one hub from the front of the matrix, one close by (the same block) when there is room
            chosen = [hubs[int(rng.integers(0, min(len(hubs), 64)))]]
            if k == 2:
                rest = [h for h in hubs if h != chosen[0]]
                chosen.append(rest[-1 - int(rng.integers(0, min(len(rest), 16)))])
            for h in chosen:
                N[j, h] = rng.choice([-1.0, 1.0])
                used.add(h)
        self.empty = sorted(self.empty)
        # coupled (unguarded) rows: same structure, with a unit pivot on top
        cand = free()
        n_coupled = int(coupled_frac * len(cand) / 3)
        for r in sorted(rng.choice(cand, size=n_coupled, replace=False)) if n_coupled else []:
            r = int(r)
            if r in used:
                continue
            hubs = [h for h in free() if h < r]
            if not hubs:
                continue
            used.add(r)
            for h in rng.choice(hubs, size=min(len(hubs), 1 + int(rng.integers(0, 2))), replace=False):
                N[r, int(h)] = rng.choice([-1.0, 1.0])
                used.add(int(h))
        D = np.ones(m)
        D[G] = 0.0
        self.L0 = np.diag(D) + N
        self.N = N
        self.dependent = sorted(set(G) - set(self.empty))
        self.n = m + n_extra
        self.A = np.zeros((m, self.n))
        self.A[:, :m] = self.L0
        self.d = np.ones(self.n)
        for r, v in self.decoupled.items():
            self.d[r] = v
        guarded = set(G)
        for name in ("t-", "t", "neg"):
            if name in self.role:
                guarded.add(self.role[name])
        self.guarded = sorted(guarded)
        self.keep = np.array([j for j in range(m) if j not in guarded], dtype=np.int64)

    # -- the matrix
    def B(self, scale=1.0):
        """A diag(scale d) A^T, formed exactly (every product and sum is an integer or a power of two times one)."""
        Ad = self.A * (self.d * scale)
        return Ad @ self.A.T

    def x_state(self, scale=1.0):
        """(x, s) with x / s = scale d: s = 1, so d is exactly x."""
        return self.d * scale, np.ones(self.n)

    # -- the expected results
    def expected_factor(self, scale_pow=0, big=BIG):
        """The guarded factor in closed form for d scaled by 4**scale_pow: unguarded columns of L0 times 2**scale_pow (the
        decoupled ones: sqrt(d_j) 2**scale_pow), guarded columns sqrt(big) e_j."""
        L = self.L0 * 2.0 ** scale_pow
        for r, v in self.decoupled.items():
            if r not in self.guarded:
                L[r, r] = np.sqrt(v) * 2.0 ** scale_pow
        for j in self.guarded:
            L[:, j] = 0.0
            L[j, j] = np.sqrt(big)
        return L

    def inexact_diag(self):
        """Rows whose expected L[j, j] = sqrt(d_j) is not exactly representable (the t+ row): compared to 2 ulp."""
        return [r for r, v in self.decoupled.items() if r not in self.guarded and np.sqrt(v) ** 2 != v]

    def reduced_solution(self, B, rhs):
        """z[keep] = B[keep, keep]^-1 rhs[keep] (what the guard computes: the guarded rows are dropped), z[guarded] = 0."""
        z = np.zeros(self.m)
        k = self.keep
        z[k] = np.linalg.solve(B[np.ix_(k, k)], rhs[k])
        return z


def host_guarded_factor(B, eps=EPS, big=BIG):
    """Right-looking guarded Cholesky on the host, with the library's rules: threshold eps * max over the non-NaN diagonal
    entries (a NaN never wins the max), a pivot p with !(p > threshold) becomes big and is counted.  O(m^3) in NumPy: for
    m up to a few hundred."""
    W = np.array(B, dtype=np.float64, copy=True)
    m = W.shape[0]
    dg = np.diag(W)
    thresh = eps * (np.nanmax(dg) if m and not np.all(np.isnan(dg)) else -np.inf)
    fixed = []
    for j in range(m):
        p = W[j, j]
        if not (p > thresh):
            p = big
            fixed.append(j)
        ljj = np.sqrt(p)
        W[j, j] = ljj
        if j + 1 < m:
            W[j + 1:, j] /= ljj
            col = W[j + 1:, j]
            W[j + 1:, j + 1:] -= np.outer(col, col)
    return np.tril(W), fixed


def auto_shift_boundary(m):
    """The largest number k of guarded pivots for which the library does NOT switch the automatic shift on: the fp64 test
    (double)k > 0.05 * (double)m of ipm_solve, small_lp.h and ipm_batch_step is false for k and true for k + 1."""
    k = int(np.floor(0.05 * m))
    while float(k + 1) <= 0.05 * float(m):
        k += 1
    while float(k) > 0.05 * float(m):
        k -= 1
    return k
