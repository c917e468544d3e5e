"""Oracle of the separable convex QP iteration (csrc/iteration_rules.h: quad_*), an extension of
tests/iteration_oracle.py by import: one Mehrotra predictor-corrector iteration with a diagonal quadratic term g, bounded and not,
restated once and run in np.longdouble (the oracle) or in float64 (the host restatement the bounds of tests/test_gpu_qp.py fall back
on), and the whole loop in float64 from the reference start.  Test infrastructure only: a helper module, not a test.

    min c.x + 1/2 x.diag(g) x,  A x = b,  0 <= x (<= u),  g >= 0

    r_c = A^T y + s - z - c - g o x          theta = x / (s + g x), on U: 1 / (s/x + z/w + g)
    objective = c.x + 1/2 x.(g o x)          everything else as iteration_oracle.py states it, with that theta and that r_c
    ONE step length (one_step=True): the affine pair and the damped pair are each replaced by their minimum

The Newton system the directions must satisfy (checked in tests/test_qp_oracle_host.py without the elimination):
    A dx = -r_b      A^T dy + ds - dz - g o dx = -r_c      s dx + x ds = -r_3      on U: dx + dw = -r_u,  z dw + w dz = -r_4
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg

import iteration_oracle as IO

LD = IO.LD


def quad_diagonal(n, seed):
    """g ~ U(0.1, 2) with g = 0 on every second column: LP and QP columns mix in one wave."""
    g = np.random.default_rng(1000 + seed).uniform(0.1, 2.0, n)
    g[1::2] = 0.0
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# one iteration, in the number type T
# ---------------------------------------------------------------------------------------------------------------------------
def _factor(A, theta, T):
    """-> the solve r -> (A diag(theta) A^T)^-1 r."""
    if T is LD:
        L = IO.cholesky(IO._normal_matrix(A, theta))
        return lambda r: IO.cholesky_solve(L, r)
    cf = scipy.linalg.cho_factor((A * theta) @ A.T, lower=True)
    return lambda r: scipy.linalg.cho_solve(cf, r)


class Problem:
    def __init__(self, A, b, c, g, u, T, transpose=True):
        self.T = T
        self.A = np.asarray(A).astype(T)
        self.AT = np.ascontiguousarray(self.A.T) if transpose else None
        self.b, self.c, self.g = (np.asarray(v, dtype=T).ravel() for v in (b, c, g))
        n = self.c.shape[0]
        u = np.full(n, np.inf) if u is None else np.asarray(u, dtype=np.float64).ravel()
        self.U = np.isfinite(u)
        self.u = np.where(self.U, u, 0.0).astype(T)
        self.n, self.nU = n, int(self.U.sum())
        self.b_norm = np.sqrt(self.b @ self.b + self.u @ self.u)
        self.c_norm = IO.norm(self.c) if T is LD else np.sqrt(self.c @ self.c)      # (LD: iteration_oracle's own summation)


def newton(P, x, y, s, w, z, eta, one_step=True, tol=None, theta_shift=0.0):
    """One iteration from (x, y, s, w, z) -> dict (the keys of iteration_oracle.iterate, plus the residual vectors rb, rc, ru and the
    corrector's complementarity terms r3c, r4c).  tol: the stop test runs first, and a converged state returns only the scalars of the
    state with converged=True.  theta_shift: a deliberately WRONG rule, theta from s + theta_shift (the "safe division" x / (s + 1e-14));
    the host files use it to show that their bounds see such a change.  0.0 leaves every bit as it is."""
    T, A, AT, U, g = P.T, P.A, P.AT, P.U, P.g
    n = P.n
    N = T(n + P.nU)
    aty = AT @ y
    rb = A @ x - P.b
    rc = aty + s - z - P.c - g * x
    ru = np.where(U, x + w - P.u, T(0))
    gap = x @ s + w @ z
    out = dict(aty=aty, rb=rb, rc=rc, ru=ru, gap=gap, mu=gap / N, rp_norm=np.sqrt(rb @ rb + ru @ ru), rd_norm=IO.norm(rc) if T is LD else np.sqrt(rc @ rc),
               objective=P.c @ x + T(0.5) * ((g * x) @ x), b_norm=P.b_norm, c_norm=P.c_norm, converged=False)
    if tol is not None and out["rp_norm"] <= tol * (1 + P.b_norm) and out["rd_norm"] <= tol * (1 + P.c_norm) and gap <= tol:
        out["converged"] = True
        return out
    st = s + T(theta_shift)
    theta = x / (st + g * x)
    theta[U] = 1 / (st[U] / x[U] + z[U] / w[U] + g[U])
    solve = _factor(A, theta, T)

    def direction(r3, r4):
        t = rc - r3 / x
        t[U] += (r4[U] - z[U] * ru[U]) / w[U]
        v = theta * t
        dy = solve(-rb - A @ v)
        atdy = AT @ dy
        dx = theta * atdy + v
        ds = -(r3 + s * dx) / x
        dw, dz = np.zeros(n, dtype=T), np.zeros(n, dtype=T)
        dw[U] = -ru[U] - dx[U]
        dz[U] = -(r4[U] + z[U] * dw[U]) / w[U]
        return dict(dx=dx, dy=dy, ds=ds, dw=dw, dz=dz, atdy=atdy)

    aff = direction(x * s, w * z)
    aap = T(IO.ratio_test(x, aff["dx"], w, aff["dw"])[0])
    aad = T(IO.ratio_test(s, aff["ds"], z, aff["dz"])[0])
    if one_step:
        aap = aad = min(aap, aad)
    mu = out["mu"]
    mu_aff = ((x + aap * aff["dx"]) @ (s + aad * aff["ds"]) + (w + aap * aff["dw"]) @ (z + aad * aff["dz"])) / N
    sigma = (mu_aff / mu) ** 3
    r3c = x * s + aff["dx"] * aff["ds"] - sigma * mu
    r4c = np.zeros(n, dtype=T)
    r4c[U] = w[U] * z[U] + aff["dw"][U] * aff["dz"][U] - sigma * mu
    cor = direction(r3c, r4c)
    ratio_p = T(IO.ratio_test(x, cor["dx"], w, cor["dw"])[0])
    ratio_d = T(IO.ratio_test(s, cor["ds"], z, cor["dz"])[0])
    eta = T(eta)
    ap, ad = min(T(1), eta * ratio_p), min(T(1), eta * ratio_d)
    if one_step:
        ap = ad = min(ap, ad)
    out.update(alpha_aff_p=aap, alpha_aff_d=aad, ratio_p=ratio_p, ratio_d=ratio_d, mu_aff=mu_aff, sigma=sigma, r3c=r3c, r4c=r4c,
               dxa=aff["dx"], dya=aff["dy"], dsa=aff["ds"], dwa=aff["dw"], dza=aff["dz"], atdya=aff["atdy"],
               dx=cor["dx"], dy=cor["dy"], ds=cor["ds"], dw=cor["dw"], dz=cor["dz"], atdy=cor["atdy"], alpha_p=ap, alpha_d=ad,
               xn=x + ap * cor["dx"], yn=y + ad * cor["dy"], sn=s + ad * cor["ds"], wn=w + ap * cor["dw"], zn=z + ad * cor["dz"],
               atyn=aty + ad * cor["atdy"])
    return out


def iterate(case, g, eta=IO.ETA, one_step=True, T=LD, theta_shift=0.0):
    """One iteration from the case's state with the diagonal g: T = LD the oracle, T = np.float64 the host restatement.
    theta_shift: see newton."""
    P = Problem(case.A, case.b, case.c, g, case.u, T)
    x, y, s, w, z = (np.asarray(v, dtype=T) for v in (case.x, case.y, case.s, case.w, case.z))
    return newton(P, x, y, s, w, z, eta, one_step, theta_shift=theta_shift)


# ---------------------------------------------------------------------------------------------------------------------------
# the whole loop in float64, from the reference start x = s = 1, y = 1 (w = z = 1 on U)
# ---------------------------------------------------------------------------------------------------------------------------
def solve64(A, b, c, g, u=None, tol=1e-8, max_iter=200, eta=IO.ETA, one_step=True):
    """-> dict(x, y, s, w, z, iterations, converged, objective, history: the objective of every iterate the stop test saw)."""
    P = Problem(A, b, c, g, u, np.float64)
    m = P.A.shape[0]
    x, s, y = np.ones(P.n), np.ones(P.n), np.ones(m)
    w = np.where(P.U, 1.0, 0.0)
    z = w.copy()
    hist = []
    for k in range(max_iter + 1):
        o = newton(P, x, y, s, w, z, eta, one_step, tol=tol)
        hist.append(float(o["objective"]))
        if o["converged"] or k == max_iter:
            return dict(x=x, y=y, s=s, w=w, z=z, iterations=k, converged=bool(o["converged"]), objective=float(o["objective"]), history=hist)
        x, y, s, w, z = o["xn"], o["yn"], o["sn"], o["wn"], o["zn"]


def stop_test_ld(A, b, c, g, u, x, y, s, w, z):
    """(rp_norm / (1 + ||(b, u_U)||), rd_norm / (1 + ||c||), gap) of a state, in longdouble: the three left-hand sides of the stop test."""
    P = Problem(A, b, c, g, u, LD, transpose=False)
    x, y, s = (np.asarray(v, dtype=LD).ravel() for v in (x, y, s))
    w = np.zeros(P.n, dtype=LD) if w is None else np.asarray(w, dtype=LD).ravel()
    z = np.zeros(P.n, dtype=LD) if z is None else np.asarray(z, dtype=LD).ravel()
    rb = P.A @ x - P.b
    rc = y @ P.A + s - z - P.c - P.g * x
    ru = np.where(P.U, x + w - P.u, LD(0))
    return (float(np.sqrt(rb @ rb + ru @ ru) / (1 + P.b_norm)), float(np.sqrt(rc @ rc) / (1 + P.c_norm)), float(x @ s + w @ z))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_qp.py (one iteration), by name: (case, g).  The dense ones are iteration_oracle's own cases.
# ---------------------------------------------------------------------------------------------------------------------------
SEED = IO.BASE_SEED
ITER_CASES = {
    "dense/129x16385b": lambda: IO.get("dense/129x16385b"),
    "dense/400x520b": lambda: IO.get("dense/400x520b"),
    "dense/520x600": lambda: IO.get("dense/520x600"),
    "sparse/130x300b": lambda: IO.sparsify(IO.interior_case(130, 300, True, SEED), 0.05),
    "sparse/60x150": lambda: IO.sparsify(IO.interior_case(60, 150, False, SEED), 0.1),
}


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, g) of that name, built once per process.  Treat both as read-only."""
    case = ITER_CASES[name]()
    return case, quad_diagonal(case.n, SEED)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The longdouble oracle of that case, computed once per process and shared: read-only."""
    return iterate(*get(name))


# ---------------------------------------------------------------------------------------------------------------------------
# the constructed problems of the whole solves (workloads.separable_qp), by name, and the float64 host loop on each
# ---------------------------------------------------------------------------------------------------------------------------
SOLVE_PROBLEMS = {          # name -> (m, n, seed, bounded, mixed)
    "300x700": (300, 700, 1, False, False),
    "300x700bm": (300, 700, 2, True, True),
    "200x520b": (200, 520, 3, True, False),
    "2560x5120": (2560, 5120, 4, False, False),
}
TOL = 1e-8


@functools.lru_cache(maxsize=None)
def problem(name):
    """(A, b, c, g, u, x_star, y_star) of that name, built once per process: read-only."""
    from interiorpointmethod_amd.workloads import separable_qp
    m, n, seed, bounded, mixed = SOLVE_PROBLEMS[name]
    return separable_qp(m, n, seed, bounded=bounded, mixed=mixed)


@functools.lru_cache(maxsize=None)
def host_loop(name):
    """solve64 of that problem at tol = 1e-8, plus x_err = ||x - x*|| / ||x*|| and obj_star, computed once per process: read-only."""
    A, b, c, g, u, xs, _ = problem(name)
    r = solve64(A, b, c, g, u, tol=TOL)
    r["x_err"] = float(np.linalg.norm(r["x"] - xs) / np.linalg.norm(xs))
    r["obj_star"] = float(c @ xs + 0.5 * (g * xs) @ xs)
    return r
