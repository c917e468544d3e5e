"""NumPy restatement of the interior-point iteration with native upper bounds 0 <= x <= u: the
arithmetic the bounded kernels of csrc/vector_ops.h and csrc/small_lp.h perform, written out on the host.  Test
infrastructure only (tests/test_bounds_host.py, tests/test_gpu_bounds.py).

U = columns with a finite u.  On U an upper slack w (x + w = u) and its dual z (>= 0) join the iterate; outside U,
w = z = 0 and the formulas reduce to the unbounded iteration of oracle/ipm_oracle.py.

    r_b = A x - b        r_c = A^T y + s - z - c        r_u = x + w - u        r_3 = x s        r_4 = w z
    theta = 1 / (s/x + z/w) on U, x/s outside          t = r_c - r_3/x + (r_4 - z r_u)/w  (second term on U only)
    (A Theta A^T) dy = -r_b - A (theta t)
    dx = theta (A^T dy) + theta t     ds = -(r_3 + s dx)/x     dw = -r_u - dx     dz = -(r_4 + z dw)/w
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ipm_oracle import cholesky_solve, guarded_cholesky  # noqa: E402  (the device's pivot guard, restated)

ETA = 0.91


def _dense(A):
    return np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=np.float64)


def _ratio(v, dv):
    neg = dv < 0
    return float(min(1.0, np.min(-v[neg] / dv[neg]))) if neg.any() else 1.0


class BoundedLP:
    def __init__(self, A, b, c, u):
        self.A = _dense(A)
        self.m, self.n = self.A.shape
        self.b = np.asarray(b, dtype=np.float64).reshape(-1)
        self.c = np.asarray(c, dtype=np.float64).reshape(-1)
        self.u = np.asarray(u, dtype=np.float64).reshape(-1)
        self.U = np.isfinite(self.u)
        self.nU = int(self.U.sum())
        self.b_norm = float(np.sqrt(self.b @ self.b + self.u[self.U] @ self.u[self.U]))
        self.c_norm = float(np.linalg.norm(self.c))

    def start(self, y0=1.0):
        """The reference start extended: x = s = 1, y = y0, w = z = 1 on U."""
        w = np.where(self.U, 1.0, 0.0)
        return np.ones(self.n), np.full(self.m, float(y0)), np.ones(self.n), w.copy(), w.copy()

    def residuals(self, x, y, s, w, z):
        U = self.U
        rb = self.A @ x - self.b
        rc = self.A.T @ y + s - z - self.c
        ru = np.where(U, x + w - np.where(U, self.u, 0.0), 0.0)
        return rb, rc, ru

    def measures(self, x, y, s, w, z):
        """(rp_norm, rd_norm, gap, mu, objective): the bounded stop-test quantities."""
        rb, rc, ru = self.residuals(x, y, s, w, z)
        gap = float(x @ s + w @ z)
        return (float(np.sqrt(rb @ rb + ru @ ru)), float(np.linalg.norm(rc)), gap, gap / (self.n + self.nU),
                float(self.c @ x))

    def converged(self, x, y, s, w, z, e1, e2, e3):
        rp, rd, gap, _, _ = self.measures(x, y, s, w, z)
        return rp <= e1 * (1.0 + self.b_norm) and rd <= e2 * (1.0 + self.c_norm) and gap <= e3

    def _theta(self, x, s, w, z):
        U = self.U
        th = x / s
        th[U] = 1.0 / (s[U] / x[U] + z[U] / w[U])
        return th

    def _direction(self, x, s, w, z, rb, rc, ru, r3, r4, L, theta):
        U = self.U
        t = rc - r3 / x
        t[U] += (r4[U] - z[U] * ru[U]) / w[U]
        v = theta * t
        rhs = -rb - self.A @ v
        dy = cholesky_solve(L, rhs)
        dx = theta * (self.A.T @ dy) + v
        ds = -(r3 + s * dx) / x
        dw = np.zeros(self.n); dz = np.zeros(self.n)
        dw[U] = -ru[U] - dx[U]
        dz[U] = -(r4[U] + z[U] * dw[U]) / w[U]
        return dx, dy, ds, dw, dz

    def _steps(self, x, s, w, z, dx, ds, dw, dz):
        U = self.U
        ap = min(_ratio(x, dx), _ratio(w[U], dw[U]))
        ad = min(_ratio(s, ds), _ratio(z[U], dz[U]))
        return ap, ad

    def predictor(self, x, y, s, w, z):
        """(dx, dy, ds, dw, dz) of the affine-scaling direction."""
        rb, rc, ru = self.residuals(x, y, s, w, z)
        theta = self._theta(x, s, w, z)
        L, _ = guarded_cholesky((self.A * theta) @ self.A.T)
        return self._direction(x, s, w, z, rb, rc, ru, x * s, w * z, L, theta)

    def iterate(self, x, y, s, w, z, eta=ETA):
        """One Mehrotra predictor-corrector step -> new (x, y, s, w, z) and a record of the step."""
        U = self.U
        rb, rc, ru = self.residuals(x, y, s, w, z)
        theta = self._theta(x, s, w, z)
        L, _ = guarded_cholesky((self.A * theta) @ self.A.T)
        r3, r4 = x * s, w * z
        dxa, dya, dsa, dwa, dza = self._direction(x, s, w, z, rb, rc, ru, r3, r4, L, theta)
        aap, aad = self._steps(x, s, w, z, dxa, dsa, dwa, dza)
        N = self.n + self.nU
        mu = float(x @ s + w @ z) / N
        mu_aff = float((x + aap * dxa) @ (s + aad * dsa) + (w[U] + aap * dwa[U]) @ (z[U] + aad * dza[U])) / N
        sigma = (mu_aff / mu) ** 3
        r3c = x * s + dxa * dsa - sigma * mu
        r4c = np.zeros(self.n)
        r4c[U] = w[U] * z[U] + dwa[U] * dza[U] - sigma * mu
        dx, dy, ds, dw, dz = self._direction(x, s, w, z, rb, rc, ru, r3c, r4c, L, theta)
        mp, md = self._steps(x, s, w, z, dx, ds, dw, dz)
        ap, ad = min(1.0, eta * mp), min(1.0, eta * md)
        rec = dict(mu=mu, mu_aff=mu_aff, sigma=sigma, alpha_aff_p=aap, alpha_aff_d=aad, alpha_p=ap, alpha_d=ad)
        return x + ap * dx, y + ad * dy, s + ad * ds, w + ap * dw, z + ad * dz, rec

    def solve(self, tol=1e-8, tol_gap=None, max_iter=500, state=None, y0=1.0):
        """Stop test first, then one step, until converged -> (x, y, s, w, z, info)."""
        e3 = tol if tol_gap is None else tol_gap
        x, y, s, w, z = self.start(y0) if state is None else [np.array(v, dtype=np.float64).reshape(-1) for v in state]
        k = 0
        status = "max_iter"
        while k < max_iter:
            if self.converged(x, y, s, w, z, tol, tol, e3):
                status = "converged"
                break
            x, y, s, w, z, _ = self.iterate(x, y, s, w, z)
            k += 1
        return x, y, s, w, z, dict(status=status, iterations=k, objective=float(self.c @ x))


def mehrotra_start(A, b, c, u):
    """Host restatement of IpmSolver._mehrotra_start_bounded (least-squares x, y; reduced cost split into s, z on U)."""
    A = _dense(A)
    m, n = A.shape
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    U = np.isfinite(u)
    L, _ = guarded_cholesky(A @ A.T)
    x = A.T @ cholesky_solve(L, b)
    y = cholesky_solve(L, A @ c)
    r = c - A.T @ y
    w = np.zeros(n); z = np.zeros(n)
    w[U] = u[U] - x[U]
    s = r.copy()
    s[U] = np.maximum(r[U], 0.0)
    z[U] = np.maximum(-r[U], 0.0)
    dp = max(-1.5 * min(x.min(), w[U].min() if U.any() else np.inf), 0.0)
    dd = max(-1.5 * min(s.min(), z[U].min() if U.any() else np.inf), 0.0)
    x = x + dp; w[U] += dp
    s = s + dd; z[U] += dd
    xs = 0.5 * float(x @ s + w[U] @ z[U])
    ss = float(s.sum() + z[U].sum())
    x = x + xs / ss; w[U] += xs / ss
    sx = float(x.sum() + w[U].sum())
    s = s + xs / sx; z[U] += xs / sx
    return x, y, s, w, z
