"""Extended-precision oracle of ONE Mehrotra predictor-corrector iteration (standard form plus native upper bounds), the
infeasibility quantities of a given iterate, and the case builders that tests/test_iteration_oracle_host.py and
tests/test_gpu_iteration_edges.py share.  Test infrastructure only: a helper module, not a test.

Everything is restated in np.longdouble (64-bit mantissa on x86), from the formulas of csrc/iteration_rules.h and
tests/bounds_oracle.py, with a Cholesky written here (LAPACK has no longdouble).  No data files, nothing from the reference project.

U = columns with a finite u; outside U, w = z = dw = dz = 0.

    r_b = A x - b        r_c = A^T y + s - z - c        r_u = x + w - u  (on U)
    theta = 1 / (s/x + z/w) on U, x/s outside           t = r_c - r_3/x + (r_4 - z r_u)/w  (second term on U only)
    (A Theta A^T) dy = -r_b - A (theta t)
    dx = theta (A^T dy) + theta t     ds = -(r_3 + s dx)/x     dw = -r_u - dx     dz = -(r_4 + z dw)/w
    predictor: r_3 = x s, r_4 = w z ; corrector: r_3 = x s + dxa dsa - sigma mu, r_4 = w z + dwa dza - sigma mu
    mu = (x.s + w.z) / (n + |U|) ; mu_aff at the affine step lengths ; sigma = (mu_aff / mu)^3
    ratio test: min(1, min over negative components of -v/dv), over (x, w) for the primal and (s, z) for the dual step
    step: alpha = min(1, eta * ratio test)  -- so alpha <= eta: a step of exactly 1.0 needs eta = 1

The cost of one oracle is the formation of A Theta A^T, m^2 n / 2 longdouble multiply-adds: 0.1 .. 3 s at the shapes below.
"""
from __future__ import annotations

import functools

import numpy as np

LD = np.longdouble
ETA = 0.91


# ---------------------------------------------------------------------------------------------------------------------------
# a case: the LP (A, b, c, u) and the state (x, y, s, w, z) one iteration starts from, all float64
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """A (m, n) dense float64; u = +inf outside the bounded set; xb, c_dual: how b and c follow from A (sparsify recomputes them):
    b = A xb, c = A^T y + s when c_dual, else independent of A."""
    FIELDS = ("A", "b", "c", "u", "x", "y", "s", "w", "z", "xb", "c_dual")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])
        self._dir = None

    def copy(self, **changes):
        kw = {f: getattr(self, f) for f in self.FIELDS}
        kw.update(changes)
        return Case(**kw)

    @property
    def m(self):
        return self.A.shape[0]

    @property
    def n(self):
        return self.A.shape[1]

    @property
    def U(self):
        return np.isfinite(self.u)

    @property
    def bounded(self):
        return bool(self.U.any())

    def ub(self):
        """What IpmSolver takes as ub= (None without a finite bound)."""
        return self.u.copy() if self.bounded else None

    def state(self):
        """Arguments of set_state."""
        return (self.x, self.y, self.s, self.w, self.z) if self.bounded else (self.x, self.y, self.s)

    def without_bounds(self):
        n = self.n
        return self.copy(u=np.full(n, np.inf), w=np.zeros(n), z=np.zeros(n))


def interior_case(m, n, bounded, seed):
    """Dense Gaussian A; x, s, w, z ~ U(0.5, 2); y ~ N(0, 1); half the columns bounded with u = x + w +- U(0, 0.3), so r_u != 0;
    b = A U(0.5, 2) and c ~ N(0, 1), so r_b != 0 and r_c != 0."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    x, s = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    y = rng.standard_normal(m)
    xb = rng.uniform(0.5, 2.0, n)
    c = rng.standard_normal(n)
    u, w, z = np.full(n, np.inf), np.zeros(n), np.zeros(n)
    if bounded:
        cols = np.sort(rng.permutation(n)[: max(1, n // 2)])
        w[cols] = rng.uniform(0.5, 2.0, cols.size)
        z[cols] = rng.uniform(0.5, 2.0, cols.size)
        u[cols] = x[cols] + w[cols] + rng.uniform(-0.3, 0.3, cols.size)
    return Case(A=A, b=A @ xb, c=c, u=u, x=x, y=y, s=s, w=w, z=z, xb=xb, c_dual=False)


def full_step_case(m, n, seed):
    """A feasible, nearly centred state without bounds: b = A x, s = (1/x) U(0.9, 1.1), c = A^T y + s."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    x = rng.uniform(0.5, 2.0, n)
    y = rng.standard_normal(m)
    s = (1.0 / x) * rng.uniform(0.9, 1.1, n)
    return Case(A=A, b=A @ x, c=A.T @ y + s, u=np.full(n, np.inf), x=x, y=y, s=s, w=np.zeros(n), z=np.zeros(n), xb=x.copy(),
                c_dual=True)


def permute_columns(case, perm):
    """Column j of the result is column perm[j] of the case: nothing but summation orders changes."""
    return case.copy(A=np.ascontiguousarray(case.A[:, perm]), c=case.c[perm], u=case.u[perm], x=case.x[perm], s=case.s[perm],
                     w=case.w[perm], z=case.z[perm], xb=case.xb[perm])


def permute_rows(case, perm):
    return case.copy(A=np.ascontiguousarray(case.A[perm, :]), b=case.b[perm], y=case.y[perm])


def _swap(n, i, j):
    perm = np.arange(n)
    perm[i], perm[j] = perm[j], perm[i]
    return perm


def place(case, primal_at=None, dual_at=None):
    """Swap columns so that the oracle's blocking column of the primal (or dual) ratio test of the STEP (the corrected direction)
    lands at the given index.  The caller recomputes the oracle on the result (iterate(result)); a permutation moves nothing but
    summation order, so the blocker moves with its column."""
    o = iterate(case)
    out = case
    if primal_at is not None:
        out = permute_columns(out, _swap(case.n, o["argmin_p"][1], primal_at))
    if dual_at is not None:
        o2 = o if primal_at is None else iterate(out)
        out = permute_columns(out, _swap(case.n, o2["argmin_d"][1], dual_at))
    return out


def sparsify(case, density, seed=0):
    """Keep about `density` of A's entries, every row and every column non-empty; b (= A xb) and, where it follows from A,
    c (= A^T y + s) recomputed; u does not depend on A.  A stays an ndarray: the caller wraps it in a csc_matrix."""
    rng = np.random.default_rng(seed)
    m, n = case.A.shape
    mask = rng.random((m, n)) < density
    for j in np.flatnonzero(~mask.any(axis=0)):
        mask[rng.integers(m), j] = True
    for i in np.flatnonzero(~mask.any(axis=1)):
        mask[i, rng.integers(n)] = True
    A = case.A * mask
    c = A.T @ case.y + case.s if case.c_dual else case.c
    return case.copy(A=A, b=A @ case.xb, c=c)


# ---------------------------------------------------------------------------------------------------------------------------
# longdouble linear algebra
# ---------------------------------------------------------------------------------------------------------------------------
def _normal_matrix(A, theta):
    """A diag(theta) A^T, lower triangle computed block row by block row and mirrored."""
    m = A.shape[0]
    Y = A * theta
    B = np.zeros((m, m), dtype=LD)
    for i0 in range(0, m, 32):
        i1 = min(m, i0 + 32)
        B[i0:i1, :i1] = np.einsum("ik,jk->ij", A[i0:i1], Y[:i1])       # both operands contiguous along k: 8x numpy's matmul here
    il = np.tril_indices(m, -1)
    B.T[il] = B[il]
    return B


def cholesky(B):
    """Lower Cholesky factor, left-looking column loop; every pivot must be positive (the cases here are well conditioned; those of
    tests/late_cases.py are not, and stay where longdouble still finds every pivot positive)."""
    m = B.shape[0]
    L = np.zeros((m, m), dtype=LD)
    for j in range(m):
        v = B[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0, "oracle Cholesky: non-positive pivot %d" % j
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def cholesky_solve(L, r):
    m = L.shape[0]
    t = np.zeros(m, dtype=LD)
    for i in range(m):
        t[i] = (r[i] - L[i, :i] @ t[:i]) / L[i, i]
    out = np.zeros(m, dtype=LD)
    for i in range(m - 1, -1, -1):
        out[i] = (t[i] - L[i + 1:, i] @ out[i + 1:]) / L[i, i]
    return out


def norm(v):
    v = np.asarray(v, dtype=LD).ravel()
    return np.sqrt((v * v).sum())


def rel(got, want):
    """||got - want|| / ||want|| in longdouble (|got - want| where want is 0)."""
    got, want = np.asarray(got, dtype=LD).ravel(), np.asarray(want, dtype=LD).ravel()
    nw = norm(want)
    return float(norm(got - want) / (nw if nw > 0 else LD(1)))


def residual_rel(got, want, data_norm):
    """Relative error of a residual norm ||A x - b|| (or ||A^T y + s - z - c||).  A residual is a difference: its own rounding error is
    about sqrt(n) eps * data_norm (data_norm = ||b|| or ||c||; 1.4e-14 data_norm for fp64 sums of 16385 terms) however small it is,
    so a relative error of 1e-12 means something only while the residual is above 1e-2 * data_norm.  Below that (full_step_case: the
    residuals are zero to rounding) the error is measured against 1e-2 * data_norm instead.  Every other case has residuals of the
    order of data_norm: the plain relative error."""
    got, want = LD(got), LD(want)
    return float(abs(got - want) / max(abs(want), LD(1e-2) * LD(data_norm)))


def ratio_test(v, dv, vb, dvb):
    """The ratio test over (v, vb) = (x, w) or (s, z): alpha = min(1, min candidates), every candidate ratio (length 2n, +inf where
    the component does not decrease), the argmin as (part, column) with part 0 = x / s and 1 = w / z, and the relative gap between
    the winning ratio and the runner-up (+inf with fewer than two candidates)."""
    n = v.shape[0]
    cand = np.full(2 * n, np.inf, dtype=LD)
    for off, a, da in ((0, v, dv), (n, vb, dvb)):
        neg = da < 0
        cand[off:off + n][neg] = -a[neg] / da[neg]
    k = int(np.argmin(cand))
    first = cand[k]
    alpha = min(LD(1), first)
    rest = np.delete(cand, k)
    second = rest.min() if rest.size else LD(np.inf)
    sep = float((second - first) / first) if np.isfinite(first) and np.isfinite(second) else np.inf
    return alpha, cand, (k // n, k % n), sep


# ---------------------------------------------------------------------------------------------------------------------------
# one iteration
# ---------------------------------------------------------------------------------------------------------------------------
def direct_solver(A, theta):
    """The normal-equations solve r -> (A Theta A^T)^-1 r of the oracle: the matrix formed and factored in longdouble."""
    L = cholesky(_normal_matrix(A, theta))
    return lambda r: cholesky_solve(L, r)


def _directions(case, solver=None):
    """Everything of the iteration that does not depend on eta (cached on the case, so the first call decides the solver).
    solver: (A, theta) in longdouble -> the solve r -> (A Theta A^T)^-1 r; None: direct_solver.  tests/late_cases.py has a second
    one, by refinement, for shapes whose longdouble formation would take minutes."""
    if case._dir is not None:
        return case._dir
    A = case.A.astype(LD)
    b, c, x, y, s, w, z = (np.asarray(v, dtype=LD) for v in (case.b, case.c, case.x, case.y, case.s, case.w, case.z))
    U = case.U
    u = np.where(U, case.u, 0.0).astype(LD)
    n, nU = case.n, int(U.sum())
    N = LD(n + nU)
    AT = np.ascontiguousarray(A.T)
    aty = AT @ y
    rb = A @ x - b
    rc = aty + s - z - c
    ru = np.where(U, x + w - u, LD(0))
    theta = x / s
    theta[U] = 1 / (s[U] / x[U] + z[U] / w[U])
    solve = (solver or direct_solver)(A, theta)

    def direction(r3, r4):
        t = rc - r3 / x
        t[U] += (r4[U] - z[U] * ru[U]) / w[U]
        v = theta * t
        dy = solve(-rb - A @ v)
        atdy = AT @ dy
        dx = theta * atdy + v
        ds = -(r3 + s * dx) / x
        dw, dz = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
        dw[U] = -ru[U] - dx[U]
        dz[U] = -(r4[U] + z[U] * dw[U]) / w[U]
        return dict(dx=dx, dy=dy, ds=ds, dw=dw, dz=dz, atdy=atdy)

    aff = direction(x * s, w * z)
    aap, cand_ap, arg_ap, sep_ap = ratio_test(x, aff["dx"], w, aff["dw"])
    aad, cand_ad, arg_ad, sep_ad = ratio_test(s, aff["ds"], z, aff["dz"])
    gap = x @ s + w @ z
    mu = gap / N
    mu_aff = ((x + aap * aff["dx"]) @ (s + aad * aff["ds"]) + (w + aap * aff["dw"]) @ (z + aad * aff["dz"])) / N
    sigma = (mu_aff / mu) ** 3
    r4c = np.zeros(n, dtype=LD)
    r4c[U] = w[U] * z[U] + aff["dw"][U] * aff["dz"][U] - sigma * mu
    cor = direction(x * s + aff["dx"] * aff["ds"] - sigma * mu, r4c)
    rp, cand_p, arg_p, sep_p = ratio_test(x, cor["dx"], w, cor["dw"])
    rd, cand_d, arg_d, sep_d = ratio_test(s, cor["ds"], z, cor["dz"])
    case._dir = dict(
        aff=aff, cor=cor, aty=aty, x=x, y=y, s=s, w=w, z=z,
        alpha_aff_p=aap, alpha_aff_d=aad, ratio_p=rp, ratio_d=rd,
        cand_aff_p=cand_ap, cand_aff_d=cand_ad, cand_p=cand_p, cand_d=cand_d,
        argmin_aff_p=arg_ap, argmin_aff_d=arg_ad, argmin_p=arg_p, argmin_d=arg_d,
        sep_aff_p=sep_ap, sep_aff_d=sep_ad, sep_p=sep_p, sep_d=sep_d,
        mu=mu, mu_aff=mu_aff, sigma=sigma, b_norm=np.sqrt(b @ b + u @ u), c_norm=norm(c), rp_norm=np.sqrt(rb @ rb + ru @ ru), rd_norm=norm(rc), gap=gap, objective=c @ x)
    return case._dir


def iterate(case, eta=ETA, solver=None):
    """One Mehrotra predictor-corrector iteration from the case's state -> dict: the affine direction (dxa, dya, dsa, dwa, dza,
    atdya = A^T dya), the corrected one (dx, dy, ds, dw, dz, atdy), the next iterate (xn, yn, sn, wn, zn, atyn = A^T yn), the
    scalars (alpha_aff_p/d, alpha_p/d, mu, mu_aff, sigma, rp_norm = ||(r_b, r_u)||, rd_norm = ||r_c||, gap, objective = c.x, the last
    four at the STARTING iterate, as the device's history records them) and, per ratio test, every candidate ratio (cand_*), the
    argmin (argmin_*: (part, column)) and the relative gap to the runner-up (sep_*).  All longdouble.  solver: see _directions."""
    d = _directions(case, solver)
    eta = LD(eta)
    ap, ad = min(LD(1), eta * d["ratio_p"]), min(LD(1), eta * d["ratio_d"])
    aff, cor = d["aff"], d["cor"]
    out = {k: v for k, v in d.items() if k not in ("aff", "cor", "x", "y", "s", "w", "z")}
    out.update(dxa=aff["dx"], dya=aff["dy"], dsa=aff["ds"], dwa=aff["dw"], dza=aff["dz"], atdya=aff["atdy"],
               dx=cor["dx"], dy=cor["dy"], ds=cor["ds"], dw=cor["dw"], dz=cor["dz"], atdy=cor["atdy"],
               alpha_p=ap, alpha_d=ad,
               xn=d["x"] + ap * cor["dx"], yn=d["y"] + ad * cor["dy"], sn=d["s"] + ad * cor["ds"],
               wn=d["w"] + ap * cor["dw"], zn=d["z"] + ad * cor["dz"], atyn=d["aty"] + ad * cor["atdy"])
    return out


# what a comparison of one iteration calls its quantities (tests/test_gpu_iteration_edges.check_iteration) -> the key of iterate()'s
# result; a scalar is named as there, with the seam it was read at in front ("aff.mu", "cor.sigma", "hist.gap")
VECTOR_KEYS = {"dxa": "dxa", "dsa": "dsa", "ATdya": "atdya", "dya": "dya", "dx": "dx", "ds": "ds", "ATdy": "atdy", "dy": "dy",
               "x": "xn", "s": "sn", "ATy": "atyn", "y": "yn", "w": "wn", "z": "zn", "dw": "dw", "dz": "dz"}


def oracle_key(quantity):
    return VECTOR_KEYS.get(quantity) or quantity.split(".")[-1]


# ---------------------------------------------------------------------------------------------------------------------------
# the infeasibility quantities of an iterate (DetArgs in csrc/iteration_rules.h) and the stop test
# ---------------------------------------------------------------------------------------------------------------------------
def infeasibility(case):
    """beta = b.y - u_U.z_U and vp = max_j (A^T y - z)_j+ ; gamma = -c.x and vd = max(||A x||_inf, max x_U); with the column attaining
    vp (col_p), the row attaining ||A x||_inf (row_d), the bounded column attaining max x_U (col_xu, None without bounds) and both
    parts of vd (ax_inf, xu_max).  All longdouble."""
    A = case.A.astype(LD)
    b, c, x, y, z = (np.asarray(v, dtype=LD) for v in (case.b, case.c, case.x, case.y, case.z))
    U = case.U
    u = np.where(U, case.u, 0.0).astype(LD)
    r = A.T @ y - z
    ax = np.abs(A @ x)
    xu = np.where(U, x, LD(0))
    return dict(beta=b @ y - u @ z, vp=max(LD(0), r.max()), col_p=int(np.argmax(r)),
                gamma=-(c @ x), vd=max(ax.max(), xu.max()), row_d=int(np.argmax(ax)), ax_inf=ax.max(), xu_max=xu.max(),
                col_xu=int(np.argmax(xu)) if U.any() else None)


def converged(case, tol):
    """The convergence test at the case's state: ||(r_b, r_u)|| <= tol (1 + ||(b, u_U)||), ||r_c|| <= tol (1 + ||c||), gap <= tol."""
    d = _directions(case) if case._dir is not None else None
    A = case.A.astype(LD)
    b, c, x, y, s, w, z = (np.asarray(v, dtype=LD) for v in (case.b, case.c, case.x, case.y, case.s, case.w, case.z))
    U = case.U
    u = np.where(U, case.u, 0.0).astype(LD)
    if d is None:
        rp = np.sqrt(((A @ x - b) ** 2).sum() + (np.where(U, x + w - u, LD(0)) ** 2).sum())
        rd = norm(A.T @ y + s - z - c)
        gap = x @ s + w @ z
    else:
        rp, rd, gap = d["rp_norm"], d["rd_norm"], d["gap"]
    return bool(rp <= tol * (1 + np.sqrt(b @ b + u @ u)) and rd <= tol * (1 + norm(c)) and gap <= tol)


def primal_fire_case(case):
    """The case with b replaced by b + t y, t such that beta = 4 vp + 1: vp <= 0.5 beta holds with a factor 2 to spare and the
    primal test of detect_fire fires at tolerance 0.5."""
    q = infeasibility(case)
    t = float(4 * q["vp"] + 1 - q["beta"]) / float(case.y @ case.y)
    return case.copy(b=case.b + t * case.y)


def dual_fire_case(case, xu_wins=False):
    """The case with b - t y (so that beta <= -1: the primal test stays silent) and c - t 1 (so that gamma = -c.x >= 4 vd + 1): the
    dual test fires at tolerance 0.5.  xu_wins: A is scaled first so that ||A x||_inf = 0.5 < max x_U, the only way the bounded part
    of vd decides (for a Gaussian A, ||A x||_inf grows like sqrt(n))."""
    if xu_wins:
        A = case.A * float(0.5 / infeasibility(case)["ax_inf"])
        case = case.copy(A=A, b=A @ case.xb)
    q = infeasibility(case)
    t_b = float(max(LD(0), q["beta"]) + 1) / float(case.y @ case.y)
    t_c = float(max(LD(0), 4 * q["vd"] + 1 - q["gamma"])) / float(case.x.sum())
    t = max(t_b, t_c)
    return case.copy(b=case.b - t * case.y, c=case.c - t)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_iteration_edges.py, by name.  tests/test_iteration_oracle_host.py asserts the preconditions of every
# one of them, so a seed below may only be replaced by one that keeps them.
# ---------------------------------------------------------------------------------------------------------------------------
DENSE_TABLE = [(1, 1, False), (3, 64, False), (5, 65, True), (130, 257, True), (300, 513, False), (400, 520, True),
               (520, 600, False), (129, 16384, False), (129, 16385, True)]
SMALL, LARGE = (130, 257), (129, 16385)
BASE_SEED = 2            # both bounded placement shapes: the blockers of the step are an x and an s component
W_BLOCKER_SEED = 1       # both shapes: the primal blocker of the step is a w component
Z_BLOCKER_SEED = 14      # 130 x 257 only: the dual blocker of the step is a z component (129 x 16385: none in seeds 1 .. 59, the
                         # z ratios stay above 0.58 where the smallest s ratio is 0.17; see raise_bound)
ZAFF_SEED, ZAFF_RAISE = 1, {257: 5.0, 16385: 15.0}      # raise_bound: the z blocker of the AFFINE dual ratio test, both shapes
FULL_STEP_SEED = 1
DENSE_SEEDS = {(1, 1): 1}   # 1 x 1: no ratio test blocks (with one column a blocked affine step makes mu_aff = 0 and sigma = 0 to
                            # rounding: nothing to compare a sigma with)


def shape_name(m, n, bounded):
    return "%dx%d%s" % (m, n, "b" if bounded else "")


def raise_bound(case, by):
    """The last bounded column's u raised by `by`: r_u = -by there, dwa ~ by and dza ~ -z (1 + by / w), so that column's z is the
    blocker of the AFFINE dual ratio test (1 / (1 + dwa / w)).  The corrected direction's second-order term takes it back."""
    j = int(np.flatnonzero(case.U)[-1])
    u = case.u.copy()
    u[j] += by
    return case.copy(u=u)


def _placements(n):
    return sorted({0, 256, n - 1} | ({16383, 16384} if n > 16384 else set()))


def _registry():
    it, fire = {}, {}
    for m, n, bd in DENSE_TABLE:
        it["dense/" + shape_name(m, n, bd)] = functools.partial(interior_case, m, n, bd, DENSE_SEEDS.get((m, n), BASE_SEED))
    for m, n in (SMALL, LARGE):
        nm = shape_name(m, n, True)
        for at in _placements(n):
            it["place/%s/p@%d" % (nm, at)] = lambda nm=nm, at=at: place(get("dense/" + nm), primal_at=at)
            it["place/%s/d@%d" % (nm, at)] = lambda nm=nm, at=at: place(get("dense/" + nm), dual_at=at)
        it["blocker/%s/w" % nm] = lambda m=m, n=n: place(interior_case(m, n, True, W_BLOCKER_SEED), primal_at=n - 1)
        it["blocker/%s/zaff" % nm] = lambda m=m, n=n: _affine_dual_at(raise_bound(interior_case(m, n, True, ZAFF_SEED), ZAFF_RAISE[n]), n - 1)
        it["sparse/" + nm] = lambda nm=nm: sparsify(get("dense/" + nm), 0.05)
        it["lock/" + shape_name(m, n, False)] = lambda nm=nm: sparsify(get("dense/" + nm).without_bounds(), 0.05)
        for bd in (False, True):
            nb = shape_name(m, n, bd)
            base = (lambda nm=nm, bd=bd: get("dense/" + nm) if bd else get("dense/" + nm).without_bounds())
            fire["primal/%s/col@%d" % (nb, n - 1)] = lambda base=base: _fire_primal_at(base(), base().n - 1)
            fire["dual/%s/row@%d" % (nb, m - 1)] = lambda base=base: _fire_dual_row_at(base(), base().m - 1)
        fire["dual/%s/xu@%d" % (nm, n - 1)] = lambda nm=nm: _fire_dual_xu_at(get("dense/" + nm), get("dense/" + nm).n - 1)
    it["blocker/%s/z" % shape_name(*SMALL, True)] = lambda: place(interior_case(*SMALL, True, Z_BLOCKER_SEED), dual_at=SMALL[1] - 1)
    it["full/" + shape_name(*LARGE, False)] = functools.partial(full_step_case, *LARGE, FULL_STEP_SEED)
    it["sparse/" + shape_name(5, 65, True)] = lambda: sparsify(get("dense/" + shape_name(5, 65, True)), 0.05)
    sp = lambda: sparsify(get("dense/" + shape_name(*SMALL, True)).without_bounds(), 0.05)
    fire["primal/sparse%s" % shape_name(*SMALL, False)] = lambda: primal_fire_case(sp())
    fire["dual/sparse%s" % shape_name(*SMALL, False)] = lambda: dual_fire_case(sp())
    return it, fire


def _affine_dual_at(case, at):
    return permute_columns(case, _swap(case.n, iterate(case)["argmin_aff_d"][1], at))


def _fire_primal_at(case, at):
    f = primal_fire_case(case)
    return permute_columns(f, _swap(f.n, infeasibility(f)["col_p"], at))


def _fire_dual_row_at(case, at):
    f = dual_fire_case(case)
    return permute_rows(f, _swap(f.m, infeasibility(f)["row_d"], at))


def _fire_dual_xu_at(case, at):
    f = dual_fire_case(case, xu_wins=True)
    return permute_columns(f, _swap(f.n, infeasibility(f)["col_xu"], at))


ITER_CASES, FIRE_CASES = _registry()


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name, built once per process; its oracle (iterate(case)) is cached on it.  Treat both as read-only."""
    return (ITER_CASES.get(name) or FIRE_CASES[name[len("fire/"):]])()
