"""Infeasible and unbounded QUADRATIC problems with known certificates (host only): the instances of the infeasibility tests of
a quadratic handle (IPM_FLAG_DETECT_QUADRATIC, detect_qp=True), built on tests/infeas_cases.py by import.

    min c.x + 1/2 x.diag(g) x,  A x = b,  0 <= x_j (<= u_j) off the free set Phi,  x_j unrestricted on Phi (g_j > 0, u_j = +inf)

Each builder returns a dict: A (dense ndarray), b, c, g (length n), ub (None or length n), free (None or int32 indices), kind
("primal_infeasible" / "dual_infeasible" / None for a NEGATIVE case, which has an optimum), the exact certificate `cert` of a positive
case and, for an unbounded one, a feasible point x0 (feasible + ray => unbounded, by construction: no external solver is needed).
The factor-model cases carry the ORIGINAL problem too (F, and `orig`: A, b, c, g, ub, cert of the original); their A, b, c, g, ub,
free are the augmented form of factor_qp_form.

detect_loop is the float64 host loop: free_qp_oracle.newton from the reference start, with the two tests of DESIGN.md 4-V on every
iterate the convergence test lets through.  CASES records, per case, the iteration at which it fires (test_qp_detect_host.py asserts
the record; test_gpu_qp_detect.py holds the device to it within the project's margin of 2 iterations)."""
import functools

import numpy as np

import free_qp_oracle as FO
import infeas_cases as IC
import iteration_oracle as IO
import qp_oracle as Q

KIND = IC.KIND
EPS = 1e-8


def _half_g(n, seed):
    """A random diagonal on half the columns (the others 0)."""
    rng = np.random.default_rng(500 + seed)
    return np.where(rng.random(n) < 0.5, rng.uniform(0.1, 2.0, n), 0.0)


def sep_primal(seed=0, m=40, n=90):
    """Separable, primal infeasible: infeas_cases.primal_infeasible_dense with a random g on half the columns (the Farkas certificate
    does not see the objective)."""
    P = IC.primal_infeasible_dense(m, n, seed)
    return dict(P, g=_half_g(n, seed), free=None)


def sep_bounded_primal():
    """Separable, infeasible only with its bounds (the certificate needs z): infeas_cases.bounded_primal_infeasible, g on half the columns."""
    P = IC.bounded_primal_infeasible()
    return dict(P, g=_half_g(P["A"].shape[1], 7), free=None)


def _ray_data(m, n, k, seed):
    """infeas_cases.bounded_dual_infeasible and the feasible point its builder draws (the same generator, the same draws)."""
    P = IC.bounded_dual_infeasible(m, n, k, seed)
    rng = np.random.default_rng(seed)
    rng.standard_normal((m, n))
    rng.random(n)
    x0 = rng.random(n) + 0.5
    x0[:k] = 0.5
    assert np.array_equal(P["A"] @ x0, P["b"])
    return P, x0


def sep_dual(seed=0, bounded=False, m=40, n=90, k=10):
    """Separable, unbounded along a ray that avoids the curvature: infeas_cases.bounded_dual_infeasible (ray d with d = 0 on the first
    k columns), g > 0 only where the ray is 0; without or with the bounds on those columns."""
    P, x0 = _ray_data(m, n, k, seed)
    g = np.zeros(n)
    g[:k] = np.random.default_rng(600 + seed).uniform(0.1, 2.0, k)
    return dict(P, ub=P["ub"] if bounded else None, g=g, free=None, x0=x0)


def sep_curved_everywhere(seed=0):
    """NEGATIVE: the LP data of sep_dual with g > 0 on EVERY column: bounded below, an optimum exists, no test may ever fire."""
    P = sep_dual(seed)
    return dict(P, g=np.random.default_rng(700 + seed).uniform(0.1, 2.0, P["A"].shape[1]), kind=None, cert=None)


def _augment(A, b, c, g, F, ub):
    from interiorpointmethod_amd import factor_qp_form
    A_, b_, c_, g_, u_, free = factor_qp_form(A, b, c, g, F, ub)
    return A_, b_, c_, g_, u_, free


def factor_primal(seed=0, m=30, n=80, k=6):
    """Factor-model (k = 6 free columns in the augmented form), primal infeasible: the constraints of primal_infeasible_dense."""
    P = IC.primal_infeasible_dense(m, n, seed)
    rng = np.random.default_rng(800 + seed)
    F, g = rng.standard_normal((n, k)) / np.sqrt(n), _half_g(n, 11 + seed)
    A_, b_, c_, g_, u_, free = _augment(P["A"], P["b"], P["c"], g, F, None)
    cert = dict(kind="primal_infeasible", y=np.concatenate([P["cert"]["y"], np.zeros(k)]), z=np.zeros(n + k))
    return dict(A=A_, b=b_, c=c_, g=g_, ub=u_, free=free, kind="primal_infeasible", cert=cert, F=F,
                orig=dict(A=P["A"], b=P["b"], c=P["c"], g=g, ub=None, cert=dict(P["cert"], y_factor=np.zeros(k))))


def _factor_ray(seed, m, n, k, kf, orthogonal):
    P, x0 = _ray_data(m, n, k, seed)
    d = P["cert"]["x"]
    rng = np.random.default_rng(900 + seed)
    F = rng.standard_normal((n, kf)) / np.sqrt(n)
    if orthogonal:
        F -= np.outer(d, d @ F) / (d @ d)                     # F^T d = 0 (to rounding: the certificate's violation says how far)
    else:
        F = np.abs(F)                                         # F > 0: F^T x != 0 for EVERY x >= 0 but 0
    g = np.zeros(n)
    g[:k] = rng.uniform(0.1, 2.0, k)
    A_, b_, c_, g_, u_, free = _augment(P["A"], P["b"], P["c"], g, F, P["ub"])
    return P, x0, d, F, g, (A_, b_, c_, g_, u_, free)


def factor_dual(seed=0, m=30, n=80, k=10, kf=6):
    """Factor-model, unbounded: the ray d of bounded_dual_infeasible (bounded columns, d = 0 there) with F^T d = 0 and g > 0 only
    where d = 0.  The augmented ray is (d, 0), the feasible point (x0, F^T x0)."""
    P, x0, d, F, g, (A_, b_, c_, g_, u_, free) = _factor_ray(seed, m, n, k, kf, True)
    cert = dict(kind="dual_infeasible", x=np.concatenate([d, np.zeros(kf)]))
    return dict(A=A_, b=b_, c=c_, g=g_, ub=u_, free=free, kind="dual_infeasible", cert=cert, x0=np.concatenate([x0, F.T @ x0]), F=F,
                orig=dict(A=P["A"], b=P["b"], c=P["c"], g=g, ub=P["ub"], cert=dict(P["cert"], t=np.zeros(kf)), x0=x0))


def factor_curved(seed=0, m=30, n=80, k=10, kf=6):
    """NEGATIVE: the same LP data with an entrywise positive F, so F^T d != 0 for EVERY ray d >= 0 of the recession cone: 1/2 |F^T x|^2
    grows quadratically along each of them and the problem is bounded below.  (A generic F with F^T d != 0 for the constructed ray
    alone does not do that: the cone keeps rays with F^T d' = 0, and the loop finds one -- as with one curved ray column.)"""
    P, x0, d, F, g, (A_, b_, c_, g_, u_, free) = _factor_ray(seed, m, n, k, kf, False)
    return dict(A=A_, b=b_, c=c_, g=g_, ub=u_, free=free, kind=None, cert=None, F=F,
                orig=dict(A=P["A"], b=P["b"], c=P["c"], g=g, ub=P["ub"]))


def one_curved_ray_column(seed=0):
    """The LP of sep_dual with curvature on ONE column of its ray only: NOT bounded -- the recession cone has other rays, and the loop
    finds one of them (status 6).  No exact certificate is carried (the ray found is the loop's own)."""
    P = sep_dual(seed)
    g = np.zeros(P["A"].shape[1])
    g[int(np.argmax(P["cert"]["x"]))] = 1.0
    return dict(P, g=g, cert=None)


def sparse_mid(kind, seed=0, m=130, n=300, k=12, density=0.05):
    """About 130 x 300 at 5 % density (beyond the one-workgroup path's 128 rows; both sparse factor paths): a dense array whose zero
    pattern the tests hand over as CSC.  kind "primal": A^T y* < 0, b.y* = 1 by a dense last row; kind "dual": a ray d with d = 0 on
    the first k columns, bounds there, closed by a dense last column."""
    rng = np.random.default_rng(1000 + seed)
    A = rng.standard_normal((m, n)) * (rng.random((m, n)) < density)
    A[np.arange(m), rng.permutation(n)[:m]] += 2.0            # full row rank
    if kind == "primal":
        ys = np.zeros(m)
        ys[-1] = 1.0
        A[-1] = -(rng.random(n) + 0.1)                         # A^T y* = A[-1] < 0
        b = rng.standard_normal(m)
        b[-1] = 1.0
        g = _half_g(n, 21 + seed)
        return dict(A=A, b=b, c=rng.random(n) + 0.1, g=g, ub=None, free=None, kind="primal_infeasible",
                    cert=dict(kind="primal_infeasible", y=ys, z=np.zeros(n)))
    d = rng.random(n) + 0.5
    d[:k] = 0.0
    A[:, -1] = -(A[:, :-1] @ d[:-1]) / d[-1]
    x0 = rng.random(n) + 0.5
    x0[:k] = 0.5
    ub = np.full(n, np.inf)
    ub[:k] = 1.0
    c = rng.standard_normal(n)
    c -= (c @ d + 1.0) * d / (d @ d)
    g = np.zeros(n)
    g[:k] = rng.uniform(0.1, 2.0, k)
    return dict(A=A, b=A @ x0, c=c, g=g, ub=ub, free=None, kind="dual_infeasible", cert=dict(kind="dual_infeasible", x=d), x0=x0)


def large_dense_qp(seed=3, k=64):
    """21 blocks of 128 rows (2688 x 5376, density 0.02): infeas_cases.large_dense with its ray taken off the first k columns (the last
    column closes A d = 0 again) and g > 0 exactly there: the fused launch and the residual stream."""
    P = IC.large_dense(seed)
    A, x0 = P["A"].copy(), P["x0"]
    d = P["cert"]["x"].copy()
    d[:k] = 0.0
    A[:, -1] = -(A[:, :-1] @ d[:-1]) / d[-1]
    c = P["c"].copy()
    c -= (c @ d + 1.0) * d / (d @ d)
    g = np.zeros(A.shape[1])
    g[:k] = np.random.default_rng(1100 + seed).uniform(0.1, 2.0, k)
    return dict(A=A, b=A @ x0, c=c, g=g, ub=None, free=None, kind="dual_infeasible", cert=dict(kind="dual_infeasible", x=d), x0=x0)


def return_target_sweep(members=64, n=40, k=4, seed=5):
    """A return-target sweep of a long-only factor-model portfolio -> list of (A as CSC, b, c, F, g), one per grid point:
    min 1/2 x.(diag(g) + F F^T) x, 1.x = 1, r.x = tau, x >= 0, tau on a grid of `members` points whose LAST THREE lie above max r:
    unattainable, so primal infeasible (Farkas: y = (-max r, 1) has A^T y = r - max r <= 0 and b.y = tau - max r > 0)."""
    from scipy import sparse
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.02, 0.12, n)
    F, g = rng.standard_normal((n, k)) * 0.1, rng.uniform(0.01, 0.05, n)
    A = sparse.csc_matrix(np.vstack([np.ones(n), r]))
    taus = np.concatenate([np.linspace(r.min() * 1.05, r.max() * 0.95, members - 3), r.max() * np.array([1.02, 1.1, 1.5])])
    return [(A, np.array([1.0, t]), np.zeros(n), F, g) for t in taus]


# name -> (builder, expected kind or None for a negative case, the iteration at which the float64 host loop's test fires / at which
# it converges).  The large case's record was taken once (its host loop takes minutes); the host test re-runs every other one.
CASES = {
    "sep-primal/0": (functools.partial(sep_primal, 0), "primal_infeasible", 14),
    "sep-primal/1": (functools.partial(sep_primal, 1), "primal_infeasible", 12),
    "sep-bounded-primal": (sep_bounded_primal, "primal_infeasible", 9),
    "sep-dual/0": (functools.partial(sep_dual, 0, False), "dual_infeasible", 11),
    "sep-dual/1": (functools.partial(sep_dual, 1, False), "dual_infeasible", 9),
    "sep-dual-bounded/0": (functools.partial(sep_dual, 0, True), "dual_infeasible", 11),
    "sep-dual-bounded/1": (functools.partial(sep_dual, 1, True), "dual_infeasible", 9),
    "factor-primal/0": (functools.partial(factor_primal, 0), "primal_infeasible", 12),
    "factor-primal/1": (functools.partial(factor_primal, 1), "primal_infeasible", 12),
    "factor-dual/0": (functools.partial(factor_dual, 0), "dual_infeasible", 10),
    "factor-dual/1": (functools.partial(factor_dual, 1), "dual_infeasible", 11),
    "one-curved-ray-column": (one_curved_ray_column, "dual_infeasible", 9),
    "sparse-primal": (functools.partial(sparse_mid, "primal"), "primal_infeasible", 12),
    "sparse-dual": (functools.partial(sparse_mid, "dual"), "dual_infeasible", 14),
    # the one-workgroup path's own edges: 1 and 8 tiles of 16 rows, n on both sides of its 512-thread stride
    "tile1/sep-dual/12x511": (functools.partial(sep_dual, 0, False, 12, 511, 10), "dual_infeasible", 9),
    "tile1/sep-primal/12x513": (functools.partial(sep_primal, 0, 12, 513), "primal_infeasible", 27),
    "tile8/sep-dual-bounded/120x513": (functools.partial(sep_dual, 1, True, 120, 513, 10), "dual_infeasible", 11),
    "tile8/factor-primal/120x511": (functools.partial(factor_primal, 0, 114, 505, 6), "primal_infeasible", 24),
    "tile8/factor-dual/128x513": (functools.partial(factor_dual, 0, 122, 507, 10, 6), "dual_infeasible", 11),
    "curved-everywhere": (sep_curved_everywhere, None, 12),
    "factor-curved/0": (functools.partial(factor_curved, 0), None, 14),
    "factor-curved/1": (functools.partial(factor_curved, 1), None, 13),
    "large-dense": (large_dense_qp, "dual_infeasible", 13),
}
POSITIVE = [nm for nm, (_, kind, _) in CASES.items() if kind is not None and nm != "large-dense"]
NEGATIVE = [nm for nm, (_, kind, _) in CASES.items() if kind is None]
SMALL = [nm for nm in CASES if nm != "large-dense"]
TILES = [nm for nm in CASES if nm.startswith("tile")]


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name, built once per process: read-only."""
    return CASES[name][0]()


def violations(P, free, x, y, z):
    """The quantities of the two tests at an iterate, in P's arithmetic -> (beta, vp, gamma, vd): vp and vd are the UNNORMALISED maxima
    (the tests compare them with eps beta and eps gamma).  State of the tests once for the host loop and the longdouble oracle."""
    T = P.T
    aty = P.AT @ y
    beta = P.b @ y - P.u[P.U] @ z[P.U]
    red = aty - z
    vp = max([T(0)] + list(red[~free]) + list(np.abs(aty[free])))
    gamma = -(P.c @ x)
    vd = max([T(0)] + list(np.abs(P.A @ x)) + list(x[P.U]) + list(P.g * np.abs(x)))
    return beta, vp, gamma, vd


def fire(beta, vp, gamma, vd, eps_p=EPS, eps_d=EPS):
    """detect_fire of csrc/iteration_rules.h -> (kind, normalisation, violation / normalisation) or None."""
    if beta > 0 and np.isfinite(beta) and vp <= eps_p * beta:
        return "primal_infeasible", beta, vp / beta
    if gamma > 0 and np.isfinite(gamma) and vd <= eps_d * gamma:
        return "dual_infeasible", gamma, vd / gamma
    return None


def detect_loop(A, b, c, g, ub=None, free=None, eps=EPS, tol=1e-8, max_iter=200, eta=IO.ETA, keep_states=False):
    """The float64 host loop with the tests: reference start, free_qp_oracle.newton, one step length where a quadratic term exists (g = 0
    everywhere is an LP handle on the device too: two step lengths, the reference's loop) -> dict(kind, k, cert, fired) with
    kind "primal_infeasible" / "dual_infeasible" (k: the iteration of the detection, cert as IpmSolver.certificate() returns it),
    "converged", "max_iter" or "nan"; fired: whether a test ever fired; keep_states: the iterates (x, y, s, w, z) up to the detection too."""
    P = Q.Problem(A, b, c, g, ub, np.float64)
    fm = FO.free_mask(free, P.n)
    x, y = np.ones(P.n), np.ones(P.A.shape[0])
    s = np.where(fm, 0.0, 1.0)
    w = np.where(P.U, 1.0, 0.0)
    z = w.copy()
    one_step = bool(np.any(P.g > 0))
    states = []
    for k in range(max_iter + 1):
        if keep_states:
            states.append((x, y, s, w, z))
        o = FO.newton(P, fm, x, y, s, w, z, eta, one_step, tol=tol)
        if o["converged"]:
            return dict(kind="converged", k=k, cert=None, fired=False, x=x, y=y, s=s, w=w, z=z)
        f = fire(*violations(P, fm, x, y, z), eps, eps)
        if f is not None:
            kind, nrm, viol = f
            cert = dict(kind=kind, normalization=float(nrm), violation=float(viol), k=k,
                        y=y / nrm if kind == "primal_infeasible" else np.zeros_like(y),
                        z=z / nrm if kind == "primal_infeasible" else np.zeros_like(z),
                        x=x / nrm if kind == "dual_infeasible" else np.zeros_like(x))
            return dict(kind=kind, k=k, cert=cert, fired=True, states=states)
        if k == max_iter:
            break
        x, y, s, w, z = o["xn"], o["yn"], o["sn"], o["wn"], o["zn"]
        if not all(np.all(np.isfinite(v)) for v in (x, y, s, w, z)):
            return dict(kind="nan", k=k + 1, cert=None, fired=False)
    return dict(kind="max_iter", k=max_iter, cert=None, fired=False)


@functools.lru_cache(maxsize=None)
def host(name):
    """detect_loop of that case, run once per process and shared: read-only."""
    P = get(name)
    return detect_loop(P["A"], P["b"], P["c"], P["g"], P["ub"], P["free"])


# ---------------------------------------------------------------------------------------------------------------------------
# ONE stop test against the longdouble oracle, where the loops change shape: a state at which one of the two tests fires with the
# quantity that decides it attained in a chosen column.  A cell is (case, g, free) like those of free_qp_oracle, built as
# iteration_oracle.primal_fire_case / dual_fire_case build the LP's: the tests fire at tolerance 0.5 with a factor 2 to spare.
# ---------------------------------------------------------------------------------------------------------------------------
LD = IO.LD


def quantities(case, g, free):
    """The two tests at the case's state in longdouble -> dict(beta, vp, gamma, vd, col_free: the free column attaining max |A^T y| and
    its signed value aty_free, col_g: the column attaining max g|x|, and the parts of both maxima)."""
    P = Q.Problem(case.A, case.b, case.c, g, case.u, LD)
    fm = FO.free_mask(free, case.n)
    x, y, z = (np.asarray(v, dtype=LD) for v in (case.x, case.y, case.z))
    beta, vp, gamma, vd = violations(P, fm, x, y, z)
    aty = P.AT @ y
    gx = P.g * np.abs(x)
    fa = np.where(fm, np.abs(aty), LD(-1))
    return dict(beta=beta, vp=vp, gamma=gamma, vd=vd, col_free=int(np.argmax(fa)) if fm.any() else None,
                aty_free=aty[int(np.argmax(fa))] if fm.any() else None, free_max=fa.max(), rest_max=max([LD(0)] + list((aty - z)[~fm])),
                col_g=int(np.argmax(gx)), gx_max=gx.max(), ax_inf=np.abs(P.A @ x).max(), xu_max=max([LD(0)] + list(x[P.U])))


def ratios(case, g, free):
    """(vp / beta, vd / gamma) of a state, +inf where the normalisation is not positive: a test fires when its ratio is <= its tolerance."""
    q = quantities(case, g, free)
    return (float(q["vp"] / q["beta"]) if q["beta"] > 0 else np.inf, float(q["vd"] / q["gamma"]) if q["gamma"] > 0 else np.inf)


def _base(m, n, bounded, free, seed=IO.BASE_SEED, x_free=None, density=None):
    case = IO.interior_case(m, n, bounded, seed)
    if density is not None:
        case = IO.sparsify(case, density)
    return FO._with_free(case, free, seed, x_free)


def curvature_cell(m, n, bounded, at, other_free, density=None, negative=True):
    """Dual fire decided by max_j g_j |x_j|, attained at column `at` -- a FREE column with x < 0 there (negative=True: the modulus
    matters) or a barrier column: ||A x||_inf is scaled to 0.5, every other g_j |x_j| to at most 0.5, max x_U <= 2, and g_at |x_at| = 3."""
    free = sorted(set(other_free) | ({at} if negative else set()))
    case, g, free = _base(m, n, bounded, free, x_free={at: -0.7} if negative else None, density=density)
    if not negative:                                           # a barrier column without a bound
        u, w, z = case.u.copy(), case.w.copy(), case.z.copy()
        u[at], w[at], z[at] = np.inf, 0.0, 0.0
        case = case.copy(u=u, w=w, z=z)
    A = case.A * float(0.5 / quantities(case, g, free)["ax_inf"])
    case = case.copy(A=A, b=A @ case.xb)
    g = g * float(0.5 / np.max(g * np.abs(case.x)))
    g[at] = 3.0 / abs(case.x[at])
    q = quantities(case, g, free)
    assert q["col_g"] == at and q["vd"] == q["gx_max"] and q["gx_max"] > max(q["ax_inf"], q["xu_max"]) + 0.9
    t_b = float(max(LD(0), q["beta"]) + 1) / float(case.y @ case.y)
    t_c = float(max(LD(0), 4 * q["vd"] + 1 - q["gamma"])) / float(case.x.sum())
    t = max(t_b, t_c)
    return case.copy(b=case.b - t * case.y, c=case.c - t), g, np.asarray(free, dtype=np.int32)


def free_dual_cell(m, n, bounded, at, other_free, sign, density=None):
    """Primal fire decided by max over the free columns of |(A^T y)_j|, attained at the free column `at` with the given sign: column
    `at` of A is scaled so that (A^T y)_at = sign (1.5 M + 1), M the largest term of every other column; then b + t y with beta = 4 vp + 1."""
    case, g, free = _base(m, n, bounded, sorted(set(other_free) | {at}), density=density)
    q = quantities(case, g, free)
    aty_at = float(case.A[:, at] @ case.y)
    A = case.A.copy()
    A[:, at] = 0.0
    M = quantities(case.copy(A=A), g, free)["vp"]
    A[:, at] = case.A[:, at] * (sign * float(1.5 * M + 1) / aty_at)
    case = case.copy(A=A, b=A @ case.xb)
    q = quantities(case, g, free)
    assert q["col_free"] == at and q["vp"] == q["free_max"] and np.sign(float(q["aty_free"])) == sign and q["free_max"] > 1.4 * q["rest_max"]
    t = float(4 * q["vp"] + 1 - q["beta"]) / float(case.y @ case.y)
    return case.copy(b=case.b + t * case.y), g, free


EDGE = {}          # name -> (builder, kind)
for _at in (0, 255, 256, 599):
    EDGE["curv/40x600/@%d" % _at] = (functools.partial(curvature_cell, 40, 600, False, _at, [300]), "dual")
    EDGE["free/40x600/@%d+" % _at] = (functools.partial(free_dual_cell, 40, 600, False, _at, [300], 1.0), "primal")
    EDGE["free/40x600/@%d-" % _at] = (functools.partial(free_dual_cell, 40, 600, False, _at, [300], -1.0), "primal")
EDGE["curv/40x600b/@256"] = (functools.partial(curvature_cell, 40, 600, True, 256, [300]), "dual")              # bounded columns interleaved
EDGE["curv/40x600b/@599barrier"] = (functools.partial(curvature_cell, 40, 600, True, 599, [300], None, False), "dual")
EDGE["free/40x600b/@256-"] = (functools.partial(free_dual_cell, 40, 600, True, 256, [300], -1.0), "primal")
EDGE["free/40x600b/@599+"] = (functools.partial(free_dual_cell, 40, 600, True, 599, [300], 1.0), "primal")
EDGE["curv/8x16500/@16420"] = (functools.partial(curvature_cell, 8, 16500, False, 16420, [3, 16383, 16384], 3.0 / 8), "dual")      # the second grid-stride trip
EDGE["free/8x16500/@16420-"] = (functools.partial(free_dual_cell, 8, 16500, False, 16420, [3, 16383, 16384], -1.0, 3.0 / 8), "primal")
EDGE["free/8x16500/@16499+"] = (functools.partial(free_dual_cell, 8, 16500, False, 16499, [3, 16384], 1.0, 3.0 / 8), "primal")
EDGE["curv/1x2/@1"] = (functools.partial(curvature_cell, 1, 2, False, 1, []), "dual")                         # m = 1: one free, one barrier column
EDGE["curv/1x2/@0barrier"] = (functools.partial(curvature_cell, 1, 2, False, 0, [1], None, False), "dual")
EDGE["free/1x2/@1+"] = (functools.partial(free_dual_cell, 1, 2, False, 1, [], 1.0), "primal")
EDGE["free/1x2/@1-"] = (functools.partial(free_dual_cell, 1, 2, False, 1, [], -1.0), "primal")


@functools.lru_cache(maxsize=None)
def edge(name):
    """(case, g, free) of that edge cell, built once per process: read-only."""
    return EDGE[name][0]()


# A test that fires first at the stop test of iteration K = 1, 2 or 3: the oracle's own trajectory from an edge cell's state (each next
# state rounded to float64, as the device holds it), the ratios of both tests at its K + 1 stop tests, and tolerances between the
# ratios of consecutive iterates, as tests/small_path_cases.delayed_fire chooses them.
DELAYED_MARGIN = 1.5


def trajectory(name, K):
    case, g, free = edge(name)
    states = [case]
    for _ in range(K):
        o = FO.iterate(states[-1], g, free)
        states.append(states[-1].copy(**{v: np.asarray(o[v + "n"], dtype=np.float64) for v in "xyswz"}))
    return states


@functools.lru_cache(maxsize=None)
def delayed(name, K):
    """-> dict(case, g, free, kind, K, tol = (eps_p, eps_d), ratios, states) or None when the cell's trajectory offers no such K: the
    named test's ratio at K must lie DELAYED_MARGIN below every earlier one, and the other test must stay silent at half its smallest
    ratio (or never have a positive normalisation)."""
    case, g, free = edge(name)
    kind = EDGE[name][1]
    which = 0 if kind == "primal" else 1
    states = trajectory(name, K)
    rs = [ratios(at, g, free) for at in states]
    mine, other = [r[which] for r in rs], [r[1 - which] for r in rs]
    if not (np.isfinite(mine[K]) and mine[K] > 0 and all(mine[K] * DELAYED_MARGIN <= v for v in mine[:K])):
        return None
    tol = [min(1e-8, 0.5 * min(other))] * 2
    tol[which] = float(np.sqrt(DELAYED_MARGIN)) * mine[K]
    if not all(0 < t < 1 for t in tol):
        return None
    return dict(case=case, g=g, free=free, kind=kind, K=K, tol=tuple(tol), ratios=rs, states=states)


# The PRIMAL test firing first at iteration K needs a state from which its ratio falls: an iterate of the host loop on a primal
# infeasible problem WITH free columns, a few iterations before its detection.  The free column that attains max |A^T y| at the
# detection is moved to the wanted place by a column swap (nothing but summation orders changes), and its sign is chosen by negating
# that column of A, c and x (a free column has no sign constraint: the same problem).
def primal_ray_problem(m, n, free, seed=0, bounded=False):
    """infeas_cases.primal_infeasible_dense with the columns of `free` made free: (A^T y*)_j = 0 there (projected), g > 0 there.
    bounded: u = 3 on every second column that is not free (bounds the certificate does not need: z stays out of it)."""
    P = IC.primal_infeasible_dense(m, n, seed)
    A, ys = P["A"].copy(), P["cert"]["y"]
    free = np.asarray(free, dtype=np.int32)
    A[:, free] -= np.outer(ys, ys @ A[:, free]) / (ys @ ys)
    g = _half_g(n, 31 + seed)
    g[free] = np.random.default_rng(1200 + seed).uniform(0.1, 2.0, free.shape[0])
    ub = None
    if bounded:
        ub = np.full(n, np.inf)
        ub[0::2] = 3.0
        ub[free] = np.inf
    return dict(A=A, b=P["b"], c=P["c"], g=g, ub=ub, free=free, kind="primal_infeasible", cert=dict(P["cert"], z=np.zeros(n)))


def _as_case(P, st):
    n = P["A"].shape[1]
    u = np.full(n, np.inf) if P["ub"] is None else P["ub"]
    return IO.Case(A=P["A"], b=P["b"], c=P["c"], u=u, x=st[0], y=st[1], s=st[2], w=st[3], z=st[4], xb=np.zeros(n), c_dual=False)


def _permuted(case, g, free, i, j):
    perm = np.arange(case.n)
    perm[[i, j]] = perm[[j, i]]
    fm = FO.free_mask(free, case.n)[perm]
    return IO.permute_columns(case, perm), g[perm], np.flatnonzero(fm).astype(np.int32)


PRIMAL_DELAYED = {}          # name -> (m, n, free columns of the problem, bounded, at, sign, K)
for _at, _K in ((_a, _k) for _a in (0, 255, 256, 599) for _k in (1, 2, 3)):
    for _sg in (1.0, -1.0):
        PRIMAL_DELAYED["free/40x600/@%d%s/K%d" % (_at, "+" if _sg > 0 else "-", _K)] = (40, 600, (100, 300, 500), False, _at, _sg, _K)
PRIMAL_DELAYED["free/40x600b/@256-/K2"] = (40, 600, (100, 301, 500), True, 256, -1.0, 2)
PRIMAL_DELAYED["free/40x600b/@599+/K1"] = (40, 600, (100, 301, 500), True, 599, 1.0, 1)
PRIMAL_DELAYED["free/8x16500/@16420-/K1"] = (8, 16500, (3, 9000, 16384), False, 16420, -1.0, 1)
PRIMAL_DELAYED["free/8x16500/@16499+/K2"] = (8, 16500, (3, 9000, 16384), False, 16499, 1.0, 2)


@functools.lru_cache(maxsize=None)
def _primal_states(m, n, free, bounded):
    P = primal_ray_problem(m, n, free, 0, bounded)
    r = detect_loop(P["A"], P["b"], P["c"], P["g"], P["ub"], P["free"], keep_states=True)
    assert r["kind"] == "primal_infeasible"
    r["q"] = [quantities(_as_case(P, st), P["g"], P["free"]) for st in r["states"]]
    return P, r


@functools.lru_cache(maxsize=None)
def primal_delayed(name):
    """-> dict(case, g, free, kind="primal", K, tol, ratios, states, kappa) like delayed(): the start state is the host loop's iterate
    K iterations before the FIRST one whose primal ratio lies DELAYED_MARGIN below the K before it (early in the solve: |y| is still
    O(1) there and (A^T y)_j is a well-conditioned sum; near the loop's own detection |y| ~ 1e6 and it is not), the attaining free
    column of the oracle's state at K swapped to `at`, its sign as asked.  kappa = sum_i |a_ij y_i| / |(A^T y)_j| of that column at
    the detection: what a float64 sum of the m products can lose against the exact one."""
    m, n, free, bounded, at, sign, K = PRIMAL_DELAYED[name]
    P, r = _primal_states(m, n, free, bounded)
    def scaled(k, lam):          # the primal ratio of iterate k once the free variable is rescaled by lam (below)
        q = r["q"][k]
        return float(max(q["rest_max"], lam * q["free_max"]) / q["beta"]) if q["beta"] > 0 else np.inf

    def lam_of(k):
        q = r["q"][k]
        return 1.0 if q["free_max"] >= 1.25 * q["rest_max"] else float(2.0 ** np.ceil(np.log2(float(1.25 * q["rest_max"] / q["free_max"]))))

    # (<= 0.75: the tolerance, sqrt(DELAYED_MARGIN) above it, stays below 1; the EARLIEST such iterate: |y| is still O(10) there)
    kd = next(k for k in range(K, len(r["q"])) if scaled(k, lam_of(k)) <= 0.75
              and all(scaled(k, lam_of(k)) * DELAYED_MARGIN * 1.05 <= scaled(j, lam_of(k)) for j in range(k - K, k)))
    case = _as_case(P, r["states"][kd - K])
    g, free = P["g"], P["free"]
    for _ in range(2):                                         # (the swap changes summation orders only: the second pass confirms the column)
        states = [case]
        for _k in range(K):
            o = FO.iterate(states[-1], g, free)
            states.append(states[-1].copy(**{v: np.asarray(o[v + "n"], dtype=np.float64) for v in "xyswz"}))
        q = quantities(states[K], g, free)
        if q["col_free"] != at:
            case, g, free = _permuted(case, g, free, q["col_free"], at)
    if np.sign(float(q["aty_free"])) != sign:
        A, c, x = case.A.copy(), case.c.copy(), case.x.copy()
        A[:, at], c[at], x[at] = -A[:, at], -c[at], -x[at]
        case = case.copy(A=A, c=c, x=x)
        states = [case]
        for _k in range(K):
            o = FO.iterate(states[-1], g, free)
            states.append(states[-1].copy(**{v: np.asarray(o[v + "n"], dtype=np.float64) for v in "xyswz"}))
        q = quantities(states[K], g, free)
    if not q["free_max"] >= 1.25 * q["rest_max"]:              # a barrier column decides vp: rescale the free variable, x_at = x'_at / lam
        lam = float(2.0 ** np.ceil(np.log2(float(1.25 * q["rest_max"] / q["free_max"]))))   # (a power of two: the same problem, exactly)
        A, c, x, g = case.A.copy(), case.c.copy(), case.x.copy(), g.copy()
        A[:, at], c[at], x[at], g[at] = lam * A[:, at], lam * c[at], x[at] / lam, lam * lam * g[at]
        case = case.copy(A=A, c=c, x=x)
        states = [case]
        for _k in range(K):
            o = FO.iterate(states[-1], g, free)
            states.append(states[-1].copy(**{v: np.asarray(o[v + "n"], dtype=np.float64) for v in "xyswz"}))
        q = quantities(states[K], g, free)
    assert q["col_free"] == at and np.sign(float(q["aty_free"])) == sign and q["vp"] == q["free_max"], (name, q["col_free"], q["aty_free"])
    rs = [ratios(st, g, free) for st in states]
    mine, other = [v[0] for v in rs], [v[1] for v in rs]
    assert np.isfinite(mine[K]) and all(mine[K] * DELAYED_MARGIN <= v for v in mine[:K]), (name, mine)
    tol = (float(np.sqrt(DELAYED_MARGIN)) * mine[K], min(1e-8, 0.5 * min(other)))
    assert all(0 < t < 1 for t in tol), (name, tol)
    kappa = float(np.abs(states[K].A[:, at] * states[K].y).sum() / abs(float(q["aty_free"])))
    return dict(case=case, g=g, free=free, kind="primal", K=K, tol=tol, ratios=rs, states=states, kappa=kappa)
