"""Oracle of the LP iteration WITH LP FREE COLUMNS (csrc/iteration_rules.h: free_lp_*), built on
tests/iteration_oracle.py the way tests/free_qp_oracle.py is: one Mehrotra predictor-corrector iteration restated once and run in
np.longdouble (the oracle) or in float64 (the host loop), and the whole loop in float64 from either start.  Test infrastructure
only: a helper module.

    min c.x,  A x = b,  0 <= x_j (<= u_j) for j NOT free,  x_j unrestricted for j free (u_j = +inf)

A free column has no s (exactly 0), no w, z, no complementarity pair; its curvature is the proximal term 1/2 rho |x - x^k|^2 centred
at the iterate, which only the Newton matrix sees:
    r_c = A^T y - c      theta = 1 / rho      q = r_3 / x := 0      v = theta r_c      dx = theta A^T dy + v      ds = 0
    no candidate in a ratio test; no term in the gap, mu, mu_aff; the pair count is n - n_free + |U|
    the LP's TWO step lengths: x += alpha_p dx, (y, s) += alpha_d (dy, ds)
With an empty free set every expression below is iteration_oracle's, evaluated in the same order on the same values: the results
are equal bit for bit (tests/test_free_lp_host.py).

The Newton system the directions must satisfy (checked there without the elimination):
    A dx = -r_b     not free: A^T dy + ds - dz = -r_c,  s dx + x ds = -r_3     free: A^T dy - rho dx = -r_c,  ds = 0
    on U: dx + dw = -r_u,  z dw + w dz = -r_4
"""
from __future__ import annotations

import functools

import numpy as np

import iteration_oracle as IO
import qp_oracle as Q
from free_qp_oracle import free_mask

LD = IO.LD
TOL = 1e-8
RHO = 1e-8          # IPM_FREE_LP_RHO_DEFAULT: what the whole solves run with
# The one-iteration comparisons run at ITER_RHO instead.  They check the ARITHMETIC of the rule against longdouble at bounds of 1e-12
# and below, and float64 can agree with longdouble only to cond(A Theta A^T) eps: with theta = 1 / rho = 1e8 on a free column beside
# theta = O(1) on the barrier columns of these interior states that is 1e8 x 1.1e-16 = 1e-8 whatever computes it (measured: the float64
# restatement below against its own longdouble run, 1.2e-8 at 1x2 and 2.1e-8 at 40x600b for rho = 1e-8; 4.6e-15 at most for rho = 0.25).
# 0.25 keeps theta = 4 among the barrier columns' theta ~ U(0.25, 4), and 1 / 0.25 is exact, so d_j == 1 / rho can be asserted bitwise.
ITER_RHO = 0.25


def newton(P, free, rho, x, y, s, w, z, eta, tol=None):
    """One iteration from (x, y, s, w, z) -> dict, the keys of iteration_oracle.iterate plus the residual vectors, theta and the
    right-hand side columns (va, qa of the predictor; v, q of the corrector).  free: boolean mask; s must be 0 there (it is forced)."""
    T, A, AT, U = P.T, P.A, P.AT, P.U
    n = P.n
    nf = ~free
    assert not (free & U).any() and nf.any() and rho > 0
    s = np.where(free, T(0), s)
    N = T(n - int(free.sum()) + P.nU)
    aty = AT @ y
    rb = A @ x - P.b
    rc = aty + s - z - P.c
    ru = np.where(U, x + w - P.u, T(0))
    gap = x[nf] @ s[nf] + w @ z
    out = dict(aty=aty, rb=rb, rc=rc, ru=ru, gap=gap, mu=gap / N, rp_norm=np.sqrt(rb @ rb + ru @ ru), rd_norm=IO.norm(rc) if T is LD else np.sqrt(rc @ rc),
               objective=P.c @ x, b_norm=P.b_norm, c_norm=P.c_norm, converged=False, free=free)
    if tol is not None and out["rp_norm"] <= tol * (1 + P.b_norm) and out["rd_norm"] <= tol * (1 + P.c_norm) and gap <= tol:
        out["converged"] = True
        return out
    xd = np.where(free, T(1), x)                       # the divisor x of q = r_3 / x and ds; a free column has neither
    theta = x / np.where(free, T(1), s)
    theta[U] = 1 / (s[U] / x[U] + z[U] / w[U])
    theta[free] = T(1) / T(rho)
    solve = Q._factor(A, theta, T)

    def direction(r3, r4):
        r3 = np.where(free, T(0), r3)
        q = r3 / xd
        t = rc - q
        t[U] += (r4[U] - z[U] * ru[U]) / w[U]
        v = theta * t
        dy = solve(-rb - A @ v)
        atdy = AT @ dy
        dx = theta * atdy + v
        ds = np.where(free, T(0), -(r3 + s * dx) / xd)
        dw, dz = np.zeros(n, dtype=T), np.zeros(n, dtype=T)
        dw[U] = -ru[U] - dx[U]
        dz[U] = -(r4[U] + z[U] * dw[U]) / w[U]
        return dict(dx=dx, dy=dy, ds=ds, dw=dw, dz=dz, atdy=atdy, v=v, q=q)

    def ratios(d):          # free columns give no candidate: their dx is hidden from the primal test, their ds is 0
        return (T(IO.ratio_test(x, np.where(free, T(0), d["dx"]), w, d["dw"])[0]), T(IO.ratio_test(s, d["ds"], z, d["dz"])[0]))

    aff = direction(x * s, w * z)
    aap, aad = ratios(aff)
    mu = out["mu"]
    mu_aff = ((x + aap * aff["dx"])[nf] @ (s + aad * aff["ds"])[nf] + (w + aap * aff["dw"]) @ (z + aad * aff["dz"])) / N
    sigma = (mu_aff / mu) ** 3
    r3c = np.where(free, T(0), x * s + aff["dx"] * aff["ds"] - sigma * mu)
    r4c = np.zeros(n, dtype=T)
    r4c[U] = w[U] * z[U] + aff["dw"][U] * aff["dz"][U] - sigma * mu
    cor = direction(r3c, r4c)
    ratio_p, ratio_d = ratios(cor)
    eta = T(eta)
    ap, ad = min(T(1), eta * ratio_p), min(T(1), eta * ratio_d)
    out.update(alpha_aff_p=aap, alpha_aff_d=aad, ratio_p=ratio_p, ratio_d=ratio_d, mu_aff=mu_aff, sigma=sigma, r3c=r3c, r4c=r4c, theta=theta,
               dxa=aff["dx"], dya=aff["dy"], dsa=aff["ds"], dwa=aff["dw"], dza=aff["dz"], atdya=aff["atdy"], va=aff["v"], qa=aff["q"],
               dx=cor["dx"], dy=cor["dy"], ds=cor["ds"], dw=cor["dw"], dz=cor["dz"], atdy=cor["atdy"], v=cor["v"], q=cor["q"], alpha_p=ap, alpha_d=ad,
               xn=x + ap * cor["dx"], yn=y + ad * cor["dy"], sn=s + ad * cor["ds"], wn=w + ap * cor["dw"], zn=z + ad * cor["dz"],
               atyn=aty + ad * cor["atdy"])
    return out


def iterate(case, free, rho=ITER_RHO, eta=IO.ETA, T=LD):
    """One iteration from the case's state with the free set: T = LD the oracle, T = np.float64 the host loop's step."""
    P = Q.Problem(case.A, case.b, case.c, np.zeros(case.n), case.u, T)
    x, y, s, w, z = (np.asarray(v, dtype=T) for v in (case.x, case.y, case.s, case.w, case.z))
    return newton(P, free_mask(free, case.n), rho, x, y, s, w, z, eta)


def mehrotra_start64(A, b, c, u=None, free=None):
    """Mehrotra's start restated for the free set in float64 (dense solves with A A^T) -> (x, y, s, w, z): on the free columns x is the
    least-squares value, unshifted and uncorrected, and s = 0; they put nothing into a minimum or a sum."""
    A = np.asarray(A, dtype=np.float64)
    b, c = np.asarray(b, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel()
    m, n = A.shape
    F = free_mask(free, n)
    Bc = ~F
    u = np.full(n, np.inf) if u is None else np.asarray(u, dtype=np.float64).ravel()
    U = np.isfinite(u)
    AAT = A @ A.T
    x = A.T @ np.linalg.solve(AAT, b)
    y = np.linalg.solve(AAT, A @ c)
    r = c - A.T @ y
    w, z = np.zeros(n), np.zeros(n)
    w[U] = u[U] - x[U]
    s = r.copy()
    s[U] = np.maximum(r[U], 0.0)
    z[U] = np.maximum(-r[U], 0.0)
    s[F] = 0.0
    dp = max(-1.5 * min(x[Bc].min(), w[U].min() if U.any() else np.inf), 0.0)
    dd = max(-1.5 * min(s[Bc].min(), z[U].min() if U.any() else np.inf), 0.0)
    x[Bc] += dp; w[U] += dp
    s[Bc] += dd; z[U] += dd
    xs = 0.5 * float(x[Bc] @ s[Bc] + w[U] @ z[U])
    sx, ss = float(x[Bc].sum() + w[U].sum()), float(s[Bc].sum() + z[U].sum())
    if not (np.isfinite(xs) and ss > 0 and sx > 0 and xs > 0):
        return np.ones(n), np.ones(m), np.where(F, 0.0, 1.0), np.where(U, 1.0, 0.0), np.where(U, 1.0, 0.0)
    x[Bc] += xs / ss; w[U] += xs / ss
    sx = float(x[Bc].sum() + w[U].sum())
    s[Bc] += xs / sx; z[U] += xs / sx
    return x, y, s, w, z


def solve64(A, b, c, u=None, free=None, rho=RHO, tol=TOL, max_iter=200, eta=IO.ETA, start="reference"):
    """The whole loop in float64 from the reference start x = 1, y = 1, s = 1 (0 on the free columns), w = z = 1 on U, or from
    mehrotra_start64 -> dict(x, y, s, w, z, iterations, converged, objective, rp_norm, rd_norm, gap)."""
    P = Q.Problem(A, b, c, np.zeros(np.asarray(c).size), u, np.float64)
    free = free_mask(free, P.n)
    if start == "mehrotra":
        x, y, s, w, z = mehrotra_start64(A, b, c, u, free)
    else:
        x, y = np.ones(P.n), np.ones(P.A.shape[0])
        s = np.where(free, 0.0, 1.0)
        w = np.where(P.U, 1.0, 0.0)
        z = w.copy()
    for k in range(max_iter + 1):
        o = newton(P, free, rho, x, y, s, w, z, eta, tol=tol)
        if o["converged"] or k == max_iter:
            return dict(x=x, y=y, s=s, w=w, z=z, iterations=k, converged=bool(o["converged"]), objective=float(o["objective"]),
                        rp_norm=float(o["rp_norm"]), rd_norm=float(o["rd_norm"]), gap=float(o["gap"]), b_norm=float(P.b_norm), c_norm=float(P.c_norm))
        x, y, s, w, z = o["xn"], o["yn"], o["sn"], o["wn"], o["zn"]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the one-iteration tests, by name: (case, free indices).  The state's s on a free column is whatever the case builder
# drew (every seam must zero it).
# ---------------------------------------------------------------------------------------------------------------------------
SEED = IO.BASE_SEED


def _with_free(case, free, x_free=None):
    """The case with those columns made free: their bounds taken off (u = +inf, w = z = 0), and x there as x_free says
    ({column: value}; 0 and negative values are legal)."""
    free = np.asarray(free, dtype=np.int32)
    u, w, z, x = case.u.copy(), case.w.copy(), case.z.copy(), case.x.copy()
    u[free], w[free], z[free] = np.inf, 0.0, 0.0
    for j, v in (x_free or {}).items():
        assert j in free
        x[j] = v
    return case.copy(u=u, w=w, z=z, x=x), free


def _smallest():
    """1 barrier column + 1 free column, m = 1: the smallest legal handle.  Seed 1: the affine step is not blocked (with ONE pair a
    blocked affine step makes mu_aff = 0 and sigma = 0 to rounding; iteration_oracle.DENSE_SEEDS)."""
    return _with_free(IO.interior_case(1, 2, False, 1), [1])


def _block_edges(bounded):
    """40 x 600: free columns on both sides of a VBLK = 256 block edge and at both ends; x = 0 and x < 0 on two of them."""
    return _with_free(IO.interior_case(40, 600, bounded, SEED), [0, 255, 256, 599], x_free={255: 0.0, 256: -0.7})


def _interleaved():
    """40 x 600 bounded: every free column sits between two bounded ones, and one bounded neighbour is nearly AT its bound:
    w = 1e-2 there with r_u = 0."""
    case = IO.interior_case(40, 600, True, SEED + 1)
    Uc = np.flatnonzero(case.U)
    mids = [int(j) + 1 for j, k in zip(Uc[:-1], Uc[1:]) if k == j + 2][:40:2]          # bounded, FREE, bounded
    assert len(mids) >= 8
    case, free = _with_free(case, mids)
    nb = int(free[3]) - 1
    w, u = case.w.copy(), case.u.copy()
    w[nb] = 1e-2
    u[nb] = case.x[nb] + w[nb]
    return case.copy(w=w, u=u), free


def _all_but_one():
    """5 x 50, every column free but column 7 (m = 5 < 49 free columns: A_Phi has full row rank, the matrix is dominated by
    A_Phi A_Phi^T / rho).  Seed 3: the affine step is not blocked (one pair: see _smallest)."""
    return _with_free(IO.interior_case(5, 50, False, 3), [j for j in range(50) if j != 7], x_free={0: 0.0, 49: -1.3})


def _sparse_mid(bounded):
    """130 x 300 at 5 % density (beyond the one-workgroup path's 128 rows): both sparse factor paths."""
    return _with_free(IO.sparsify(IO.interior_case(130, 300, bounded, SEED), 0.05), [0, 17, 255, 256, 299], x_free={17: 0.0, 256: -0.4})


def _sparse_wide():
    """8 x 16500 with about three entries per column: n > MAXPART * VBLK = 16384, so the grid-stride loop of the vector kernels makes a
    second trip; free columns in the first trip, at the stride column and in the second trip."""
    return _with_free(IO.sparsify(IO.interior_case(8, 16500, False, SEED), 3.0 / 8), [3, 16383, 16384], x_free={16384: -0.5})


ITER_CASES = {
    "1x2": _smallest,
    "40x600": functools.partial(_block_edges, False),
    "40x600b": functools.partial(_block_edges, True),
    "40x600b-interleaved": _interleaved,
    "5x50-all-but-one": _all_but_one,
    "sparse/130x300": functools.partial(_sparse_mid, False),
    "sparse/130x300b": functools.partial(_sparse_mid, True),
    "sparse/8x16500": _sparse_wide,
}


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, free) of that name, built once per process: read-only."""
    return ITER_CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name, rho=ITER_RHO):
    """The longdouble oracle of that case, computed once per process and shared: read-only."""
    case, free = get(name)
    return iterate(case, free, rho)


# ---------------------------------------------------------------------------------------------------------------------------
# the constructed problems of the whole solves (workloads.free_lp), by name, and the float64 host loop on each
# ---------------------------------------------------------------------------------------------------------------------------
SOLVE_PROBLEMS = {          # name -> (m, n, n_free, seed, bounded, dependent)
    "1x2": (1, 2, 1, 7, False, False),
    "8x20": (8, 20, 3, 7, False, False),
    "40x130b": (40, 130, 10, 7, True, False),
    "40x130dep": (40, 130, 10, 7, False, True),
    "200x520": (200, 520, 20, 7, False, False),
    "1921x4096": (1921, 4096, 48, 7, False, False),          # 16 blocks of 128 rows: the smallest dense shape on the fused launch
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(A, b, c, free, u, x_star, y_star, s_star) of that name, built once per process: read-only."""
    from interiorpointmethod_amd.workloads import free_lp
    m, n, nf, seed, bounded, dependent = SOLVE_PROBLEMS[name]
    return free_lp(m, n, nf, seed, bounded=bounded, dependent=dependent)


@functools.lru_cache(maxsize=None)
def host_loop(name, start="reference", rho=RHO):
    """solve64 of that problem at tol = 1e-8, plus x_err = ||x - x*|| / ||x*||, y_err and obj_star: read-only."""
    A, b, c, free, u, xs, ys, ss = problem(name)
    r = solve64(A, b, c, u, free, rho=rho, tol=TOL, start=start)
    r["x_err"] = float(np.linalg.norm(r["x"] - xs) / np.linalg.norm(xs))
    r["y_err"] = float(np.linalg.norm(r["y"] - ys) / np.linalg.norm(ys))
    r["obj_star"] = float(c @ xs)
    return r
