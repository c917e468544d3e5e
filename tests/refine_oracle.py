"""NumPy restatement of the iterative refinement of one normal-equations solve (csrc/iteration_rules.h: refine_decide; DESIGN.md
4-I), its input families and its extended-precision reference.  Shared by tests/test_refine_oracle_host.py (CPU) and
tests/test_gpu_refine.py.

The rule, for one solve with right-hand side t, result dy = B~^-1 t and a = A^T dy.  Round j = 1 .. k:
  1. r = t - A (d o a), rho_j = ||r||_2;
  2. rho_j is 0 or not finite: the rounds end;
  3. j > 1 and rho_j > rho_{j-1}: (dy, a) restored from the copy taken before the previous correction, a revert, the rounds end;
  4. j > 1 and rho_j > rho_{j-1} / 2: the rounds end, the previous correction stays;
  5. otherwise copy (dy, a), delta = B~^-1 r, dy += delta, a += A^T delta.
B~ is what the library factors: fl(A diag(d) A^T) + shift * max diag on the diagonal, pivots at or below eps * max diag replaced
by big (guard_cases.host_guarded_factor), rounded through a Cholesky.  The oracle uses LAPACK-free NumPy for the guarded factor and
scipy's triangular solves, not the library's kernels: it shares the rule and the arithmetic model, not the summation order.
"""
import numpy as np
from scipy.linalg import solve_triangular

from guard_cases import BIG, EPS, host_guarded_factor

LD = np.longdouble


class Factor:
    """B~ = L L^T of B = fl(A diag(d) A^T) with the library's shift and pivot guard."""

    def __init__(self, A, d, shift=0.0, eps=EPS, big=BIG):
        A = np.asarray(A, dtype=np.float64)
        B = (A * d) @ A.T
        B = 0.5 * (B + B.T)
        mx = float(np.max(np.diag(B)))
        if shift:
            B = B + shift * mx * np.eye(B.shape[0])
        self.L, self.fixed = host_guarded_factor(B, eps=eps, big=big)

    def solve(self, r):
        z = solve_triangular(self.L, r, lower=True)
        return solve_triangular(self.L.T, z, lower=False)


def refine(A, d, t, k, solve):
    """The rule in float64 -> dict(dy, a, rho (every rho_j measured), applied, half, reverts, dy0 (the unrefined solve)).
    `solve`: r -> B~^-1 r."""
    A = np.asarray(A, dtype=np.float64)
    dy = solve(t)
    a = A.T @ dy
    out = dict(dy0=dy.copy(), rho=[], applied=0, half=0, reverts=0)
    keep = None
    for j in range(1, k + 1):
        r = t - A @ (d * a)
        rho = float(np.sqrt(r @ r))
        out["rho"].append(rho)
        if not (rho > 0.0) or not np.isfinite(rho):
            break
        if j > 1 and rho > out["rho"][-2]:
            dy, a = keep
            out["reverts"] += 1
            break
        if j > 1 and rho > 0.5 * out["rho"][-2]:
            out["half"] += 1
            break
        keep = (dy.copy(), a.copy())
        delta = solve(r)
        dy = dy + delta
        a = a + A.T @ delta
        out["applied"] += 1
    out["dy"], out["a"] = dy, a
    return out


def residual_norm(A, d, t, dy):
    """||t - A D^2 A^T dy||_2 in extended precision."""
    A, d, t, dy = (np.asarray(v, dtype=LD) for v in (A, d, t, dy))
    r = t - A @ (d * (A.T @ dy))
    return float(np.sqrt(r @ r))


def reference(A, d, t, max_rounds=60):
    """The solution of (A D^2 A^T) y = t to extended precision: a double solve with the UNSHIFTED double factor, refined with
    residuals formed in np.longdouble until the iterate is stationary (relative change below 2^-70, or no longer shrinking)."""
    f = Factor(A, d)
    assert not f.fixed, "the reference needs a nonsingular matrix"
    Al, dl, tl = (np.asarray(v, dtype=LD) for v in (A, d, t))
    y = np.asarray(f.solve(np.asarray(t, dtype=np.float64)), dtype=LD)
    last = np.inf
    for _ in range(max_rounds):
        r = tl - Al @ (dl * (Al.T @ y))
        dlt = np.asarray(f.solve(np.asarray(r, dtype=np.float64)), dtype=LD)
        y = y + dlt
        step = float(np.sqrt(dlt @ dlt) / np.sqrt(y @ y))
        if step < 2.0 ** -70 or step >= last:
            break
        last = step
    return y


def forward_error(dy, ref):
    e = np.asarray(dy, dtype=LD) - ref
    return float(np.sqrt(e @ e) / np.sqrt(ref @ ref))


# ---- the input families -----------------------------------------------------------------------------------------------------
# (name, spread exponent p, shift): A ~ N(0, 1); d the quotient of two U(0.5, 1.5) draws times exp(U(-ln 10^p, ln 10^p))
FAMILIES = [("p0-shift1e-6", 0, 1e-6), ("p4-shift1e-8", 4, 1e-8), ("p4-shift0", 4, 0.0), ("p8-shift0", 8, 0.0), ("p8-shift1e-12", 8, 1e-12)]
SIZES = [(m, n) for m in (130, 257) for n in (2 * m, 2 * m + 1, m + 43)]
_SEED = 20260419


class Case:
    def __init__(self, family, m, n):
        name, p, shift = next(f for f in FAMILIES if f[0] == family)
        rng = np.random.default_rng([_SEED, p, m, n, int(shift != 0.0)])
        self.family, self.m, self.n, self.p, self.shift = name, m, n, p, shift
        self.A = rng.standard_normal((m, n))
        d = rng.uniform(0.5, 1.5, n) / rng.uniform(0.5, 1.5, n)
        if p:
            lim = p * np.log(10.0)
            d = d * np.exp(rng.uniform(-lim, lim, n))
        self.d = d
        self.t = rng.standard_normal(m)
        self.name = "%s/%dx%d" % (name, m, n)

    def cond(self):
        return float(np.linalg.cond((self.A * self.d) @ self.A.T))


_cache = {}


def _evaluate(c):
    """Fills in the reference and the oracle's runs at k = 0, 1, 2 for the case's (A, d, t, shift)."""
    c.ref = reference(c.A, c.d, c.t)
    f = Factor(c.A, c.d, shift=c.shift)
    c.fixed = list(f.fixed)
    c.runs = {k: refine(c.A, c.d, c.t, k, f.solve) for k in (0, 1, 2)}
    c.err = {k: forward_error(c.runs[k]["dy"], c.ref) for k in (0, 1, 2)}
    c.err2_other = forward_error(refine(c.A, c.d, c.t, 2, other_solver(c))["dy"], c.ref)
    return c


def get(family, m, n):
    """The case with its reference and the oracle's runs at k = 0, 1, 2, computed once and shared."""
    key = (family, m, n)
    if key not in _cache:
        _cache[key] = _evaluate(Case(family, m, n))
    return _cache[key]


def bounded_columns(n):
    U = np.zeros(n, dtype=bool)
    U[::3] = True
    return U


def get_theta(family, m, n):
    """The same case with d replaced, on every third column, by theta = 1 / (1/d + 1): what a bounded handle computes from the
    state x = d q, s = w = z = q (q a power of two) in the device's own expression 1 / (s/x + z/w).  Evaluated like any other
    case (its own reference, oracle runs and predicate), computed once and shared."""
    key = (family, m, n, "theta")
    if key not in _cache:
        c = Case(family, m, n)
        U = bounded_columns(n)
        c.d = np.where(U, 1.0 / (1.0 / c.d + 1.0), c.d)
        c.name += "/theta"
        _cache[key] = _evaluate(c)
    return _cache[key]


# What the GPU test asserts of the device, asked of the oracle alone first (test_refine_oracle_host.py):
#   * the error at k = 0 exceeds GAIN x the error at k = 2;
#   * the device's error at k = 2 is within ORACLE_MARGIN x the oracle's, "a different factorization and summation order".  Of the
#     oracle alone: its error at k = 2 under a second, equally legitimate double-precision factorization (other_solver) agrees
#     with the first within STABLE = sqrt(ORACLE_MARGIN).  Where two host factorizations already differ by more than the square
#     root of the margin, the bound cannot be asserted of a third.
# A family / size that misses either is dropped by this predicate, for the CPU test and the GPU test alike.
GAIN = 100.0
ORACLE_MARGIN = 16.0
STABLE = 4.0


def other_solver(c):
    """B~ from the columns in reverse order, LAPACK's blocked Cholesky."""
    A, d = c.A[:, ::-1], c.d[::-1]
    B = (A * d) @ A.T
    B = 0.5 * (B + B.T)
    if c.shift:
        B = B + c.shift * float(np.max(np.diag(B))) * np.eye(c.m)
    L = np.linalg.cholesky(B)
    return lambda r: solve_triangular(L.T, solve_triangular(L, r, lower=True), lower=False)


def stable(c):
    return max(c.err[2], c.err2_other) <= STABLE * min(c.err[2], c.err2_other)


def oracle_meets(c):
    return c.err[0] > GAIN * c.err[2] and not c.fixed and stable(c)


def kept_cases():
    return [(f[0], m, n) for f in FAMILIES for (m, n) in SIZES if oracle_meets(get(f[0], m, n))]


# ---- the constructed case of rules 3 and 4 ----------------------------------------------------------------------------------
class DuplicatedRow:
    """A (m x n) whose row `dup` is a copy of row `src` (src < dup): the pivot of `dup` cancels to rounding and the guard replaces
    it by big (eps is raised to 1e-12 so that the rounding residue of the cancellation is below the threshold whatever the
    summation order).  consistent(): a right-hand side in the range (t[dup] = t[src]); inconsistent(): t[dup] != t[src], whose
    residual cannot fall below |t[dup] - t[src]| / sqrt(2)."""
    eps = 1e-12

    def __init__(self, m=40, n=90, src=7, dup=23, seed=5):
        rng = np.random.default_rng([_SEED, m, n, seed])
        self.m, self.n, self.src, self.dup = m, n, src, dup
        self.A = rng.standard_normal((m, n))
        self.A[dup] = self.A[src]
        self.d = rng.uniform(0.5, 1.5, n) / rng.uniform(0.5, 1.5, n)
        self._t = rng.standard_normal(m)

    def consistent(self):
        t = self._t.copy()
        t[self.dup] = t[self.src]
        return t

    def inconsistent(self):
        t = self._t.copy()
        t[self.dup] = t[self.src] + 1.0
        return t
