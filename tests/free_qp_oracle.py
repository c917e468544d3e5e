"""Oracle of the separable-QP iteration WITH FREE COLUMNS (csrc/iteration_rules.h: free_*), an extension of
tests/qp_oracle.py by import: one Mehrotra predictor-corrector iteration restated once and run in np.longdouble (the oracle) or in
float64 (the host loop), and the whole loop in float64 from the reference start.  Test infrastructure only: a helper module.

    min c.x + 1/2 x.diag(g) x,  A x = b,  0 <= x_j (<= u_j) for j NOT free,  x_j unrestricted for j free (g_j > 0, u_j = +inf)

A free column has no s (exactly 0), no w, z, no complementarity pair:
    r_c = A^T y - c - g o x      theta = 1 / g      q = r_3 / x := 0      v = theta r_c      dx = theta A^T dy + v      ds = 0
    no candidate in a ratio test; no term in the gap, mu, mu_aff; the pair count is n - n_free + |U|
Everything else as qp_oracle.newton states it (one step length included).  With an empty free set every expression below is
qp_oracle.newton's, evaluated in the same order on the same values: the results are equal bit for bit (tests/test_free_qp_host.py).

The Newton system the directions must satisfy (checked there without the elimination):
    A dx = -r_b     not free: A^T dy + ds - dz - g o dx = -r_c,  s dx + x ds = -r_3     free: A^T dy - g o dx = -r_c,  ds = 0
    on U: dx + dw = -r_u,  z dw + w dz = -r_4
"""
from __future__ import annotations

import functools

import numpy as np

import iteration_oracle as IO
import qp_oracle as Q

LD = IO.LD
TOL = Q.TOL


def free_mask(free, n):
    """None, indices or a boolean mask -> a boolean mask of length n."""
    mask = np.zeros(n, dtype=bool)
    if free is None:
        return mask
    f = np.asarray(free)
    if f.dtype == np.bool_:
        return f.reshape(-1).copy()
    mask[f.astype(np.int64).reshape(-1)] = True
    return mask


def newton(P, free, x, y, s, w, z, eta, one_step=True, tol=None):
    """One iteration from (x, y, s, w, z) -> dict, the keys of qp_oracle.newton plus theta, the right-hand side columns (va, qa of
    the predictor; v, q of the corrector) and free.  free: boolean mask; s must be 0 there (it is forced)."""
    T, A, AT, U, g = P.T, P.A, P.AT, P.U, P.g
    n = P.n
    nf = ~free
    assert not (free & U).any() and np.all(g[free] > 0) and nf.any()
    s = np.where(free, T(0), s)
    N = T(n - int(free.sum()) + P.nU)
    aty = AT @ y
    rb = A @ x - P.b
    rc = aty + s - z - P.c - g * x
    ru = np.where(U, x + w - P.u, T(0))
    gap = x[nf] @ s[nf] + w @ z
    out = dict(aty=aty, rb=rb, rc=rc, ru=ru, gap=gap, mu=gap / N, rp_norm=np.sqrt(rb @ rb + ru @ ru), rd_norm=IO.norm(rc) if T is LD else np.sqrt(rc @ rc),
               objective=P.c @ x + T(0.5) * ((g * x) @ x), b_norm=P.b_norm, c_norm=P.c_norm, converged=False, free=free)
    if tol is not None and out["rp_norm"] <= tol * (1 + P.b_norm) and out["rd_norm"] <= tol * (1 + P.c_norm) and gap <= tol:
        out["converged"] = True
        return out
    xd = np.where(free, T(1), x)                       # the divisor x of q = r_3 / x and ds; a free column has neither
    den = np.where(free, T(1), s + g * x)
    theta = x / den
    theta[U] = 1 / (s[U] / x[U] + z[U] / w[U] + g[U])
    theta[free] = 1 / g[free]
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
    if one_step:
        aap = aad = min(aap, aad)
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
    if one_step:
        ap = ad = min(ap, ad)
    out.update(alpha_aff_p=aap, alpha_aff_d=aad, ratio_p=ratio_p, ratio_d=ratio_d, mu_aff=mu_aff, sigma=sigma, r3c=r3c, r4c=r4c, theta=theta,
               dxa=aff["dx"], dya=aff["dy"], dsa=aff["ds"], dwa=aff["dw"], dza=aff["dz"], atdya=aff["atdy"], va=aff["v"], qa=aff["q"],
               dx=cor["dx"], dy=cor["dy"], ds=cor["ds"], dw=cor["dw"], dz=cor["dz"], atdy=cor["atdy"], v=cor["v"], q=cor["q"], alpha_p=ap, alpha_d=ad,
               xn=x + ap * cor["dx"], yn=y + ad * cor["dy"], sn=s + ad * cor["ds"], wn=w + ap * cor["dw"], zn=z + ad * cor["dz"],
               atyn=aty + ad * cor["atdy"])
    return out


def iterate(case, g, free, eta=IO.ETA, one_step=True, T=LD):
    """One iteration from the case's state with the diagonal g and the free set: T = LD the oracle, T = np.float64 the host loop's step."""
    P = Q.Problem(case.A, case.b, case.c, g, case.u, T)
    x, y, s, w, z = (np.asarray(v, dtype=T) for v in (case.x, case.y, case.s, case.w, case.z))
    return newton(P, free_mask(free, case.n), x, y, s, w, z, eta, one_step)


def solve64(A, b, c, g, u=None, free=None, tol=TOL, max_iter=200, eta=IO.ETA, one_step=True):
    """The whole loop in float64 from the reference start x = 1, y = 1, s = 1 (0 on the free columns), w = z = 1 on U
    -> dict(x, y, s, w, z, iterations, converged, objective)."""
    P = Q.Problem(A, b, c, g, u, np.float64)
    free = free_mask(free, P.n)
    x, y = np.ones(P.n), np.ones(P.A.shape[0])
    s = np.where(free, 0.0, 1.0)
    w = np.where(P.U, 1.0, 0.0)
    z = w.copy()
    for k in range(max_iter + 1):
        o = newton(P, free, x, y, s, w, z, eta, one_step, tol=tol)
        if o["converged"] or k == max_iter:
            return dict(x=x, y=y, s=s, w=w, z=z, iterations=k, converged=bool(o["converged"]), objective=float(o["objective"]))
        x, y, s, w, z = o["xn"], o["yn"], o["sn"], o["wn"], o["zn"]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of the one-iteration tests, by name: (case, g, free indices).  g > 0 on every free column; the state's s there is
# whatever the case builder drew (every seam must zero it).
# ---------------------------------------------------------------------------------------------------------------------------
SEED = IO.BASE_SEED


def _with_free(case, free, seed=SEED, x_free=None):
    """The case with those columns made free: their bounds taken off (u = +inf, w = z = 0), g from qp_oracle.quad_diagonal with
    fresh positive entries on the free columns, and x there as x_free says ({column: value}; 0 and negative values are legal)."""
    free = np.asarray(free, dtype=np.int32)
    g = Q.quad_diagonal(case.n, seed)
    g[free] = np.random.default_rng(2000 + seed).uniform(0.1, 2.0, free.shape[0])
    u, w, z, x = case.u.copy(), case.w.copy(), case.z.copy(), case.x.copy()
    u[free], w[free], z[free] = np.inf, 0.0, 0.0
    for j, v in (x_free or {}).items():
        assert j in free
        x[j] = v
    return case.copy(u=u, w=w, z=z, x=x), g, free


def _smallest():
    """1 barrier column + 1 free column, m = 1: the smallest legal handle.  Seed 2: the affine step is not blocked (with ONE pair a
    blocked affine step makes mu_aff = 0 and sigma = 0 to rounding: nothing to compare a sigma with; iteration_oracle.DENSE_SEEDS)."""
    c = IO.interior_case(1, 2, False, 2)
    return _with_free(c, [1])


def _block_edges(bounded):
    """40 x 600: free columns on both sides of a VBLK = 256 block edge and at both ends; x = 0 and x < 0 on two of them."""
    return _with_free(IO.interior_case(40, 600, bounded, SEED), [0, 255, 256, 599], x_free={255: 0.0, 256: -0.7})


def _interleaved():
    """40 x 600 bounded: every free column sits between two bounded ones, and one bounded neighbour (of free column j0) is nearly AT
    its bound: w = 1e-2 there with r_u = 0 (an interior state cannot sit on it)."""
    case = IO.interior_case(40, 600, True, SEED + 1)
    Uc = np.flatnonzero(case.U)
    mids = [int(j) + 1 for j, k in zip(Uc[:-1], Uc[1:]) if k == j + 2][:40:2]          # bounded, FREE, bounded
    assert len(mids) >= 8
    case, g, free = _with_free(case, mids)
    nb = int(free[3]) - 1
    w, u = case.w.copy(), case.u.copy()
    w[nb] = 1e-2
    u[nb] = case.x[nb] + w[nb]
    return case.copy(w=w, u=u), g, free


def _all_but_one():
    """5 x 50, every column free but column 7.  Seed 5: the affine step is not blocked (one pair: see _smallest)."""
    c = IO.interior_case(5, 50, False, 5)
    return _with_free(c, [j for j in range(50) if j != 7], x_free={0: 0.0, 49: -1.3})


def _sparse_mid(bounded):
    """130 x 300 at 5 % density (beyond the one-workgroup path's 128 rows): both sparse factor paths."""
    return _with_free(IO.sparsify(IO.interior_case(130, 300, bounded, SEED), 0.05), [0, 17, 255, 256, 299], x_free={17: 0.0, 256: -0.4})


def _sparse_wide():
    """8 x 16500 with about three entries per column: n > MAXPART * VBLK = 16384, so the grid-stride loop of the vector kernels makes a
    second trip; free columns in the first trip, at the stride column and in the second trip."""
    c = IO.sparsify(IO.interior_case(8, 16500, False, SEED), 3.0 / 8)
    return _with_free(c, [3, 16383, 16384, 16420, 16499], x_free={16420: -0.5, 16499: 0.0})


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
    """(case, g, free) of that name, built once per process: read-only."""
    return ITER_CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The longdouble oracle of that case, computed once per process and shared: read-only."""
    return iterate(*get(name))


# ---------------------------------------------------------------------------------------------------------------------------
# the constructed factor-model problems of the whole solves (workloads.factor_qp), by name, and the float64 host loop on each
# ---------------------------------------------------------------------------------------------------------------------------
SOLVE_PROBLEMS = {          # name -> (m, n, k, seed, bounded)
    "1x64k8b": (1, 64, 8, 7, True),
    "3x20k2": (3, 20, 2, 7, False),
    "40x130k8b": (40, 130, 8, 7, True),
    "300x700k64": (300, 700, 64, 7, False),
    "200x520k16": (200, 520, 16, 7, False),
    "2560x5120k64": (2560, 5120, 64, 7, False),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(A, b, c, g, F, u, x_star, y_star) of that name, built once per process: read-only."""
    from interiorpointmethod_amd.workloads import factor_qp
    m, n, k, seed, bounded = SOLVE_PROBLEMS[name]
    return factor_qp(m, n, k, seed, bounded=bounded)


@functools.lru_cache(maxsize=None)
def host_loop(name):
    """solve64 of that problem's augmented form (factor_qp_form) at tol = 1e-8, plus x_err = ||x - x*|| / ||x*|| and y_err over the
    ORIGINAL problem's n columns and m rows, t_err = ||t - F^T x*|| / ||F^T x*|| and obj_star: read-only."""
    from interiorpointmethod_amd import factor_qp_form
    A, b, c, g, F, u, xs, ys = problem(name)
    A_, b_, c_, g_, u_, free = factor_qp_form(A, b, c, g, F, u)
    r = solve64(A_, b_, c_, g_, u_, free, tol=TOL)
    m, n = A.shape
    ts = F.T @ xs
    r["x_err"] = float(np.linalg.norm(r["x"][:n] - xs) / np.linalg.norm(xs))
    r["y_err"] = float(np.linalg.norm(r["y"][:m] - ys) / np.linalg.norm(ys))
    r["t_err"] = float(np.linalg.norm(r["x"][n:] - ts) / np.linalg.norm(ts))
    r["obj_star"] = float(c @ xs + 0.5 * (g * xs) @ xs + 0.5 * ts @ ts)
    return r
