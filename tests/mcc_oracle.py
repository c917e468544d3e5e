"""Extended-precision oracle of ONE interior-point iteration with up to K of Gondzio's centrality-corrector rounds behind Mehrotra's
corrector (csrc/iteration_rules.h: mcc_*), and the cells tests/test_mcc_oracle_host.py and tests/test_gpu_mcc.py
share.  Test infrastructure only: a helper module, not a test.

Built from the pieces of tests/iteration_oracle.py: Mehrotra's part of the iteration is iteration_oracle.iterate itself (so K = 0
IS that oracle), the rounds re-use its Case, _normal_matrix, cholesky, cholesky_solve and ratio_test.  np.longdouble throughout;
prec=np.float64 runs the same statements in fp64 with LAPACK's Cholesky (the restatement the host test holds against the oracle).

One round, from the direction D = (dx, dy, ds, dw, dz) with complementarity terms r3, r4 and step lengths a_p, a_d (sm = sigma mu):
    a~ = min(1, a + delta)                                v = (x + a~_p dx)(s + a~_d ds)           (and (w, z, dw, dz) on U)
    t  = max(clip(v, beta_min sm, beta_max sm) - v, -beta_max sm)
    r3g = r3 - t, r4g = r4 - t4  ->  the corrector's direction formulas with this iteration's factor  ->  candidate, ratio tests
    a^ = min(1, eta ratio) ; margin = a^_p + a^_d - a_p - a_d - gamma delta ; accept iff margin >= 0
    accepted: (D, r3, r4, a) <- the candidate's ; rejected: the iteration keeps what it had and runs no further round
"""
from __future__ import annotations

import numpy as np

import iteration_oracle as IO

LD = IO.LD
DELTA, GAMMA, BETA_MIN, BETA_MAX = 0.1, 0.1, 0.1, 10.0       # csrc/iteration_rules.h: MCC_*
MAX_K = 3                                                     # what the cells are computed for; K < MAX_K is a prefix of it


class _Base:
    """What every direction of an iteration shares: the residuals, theta and the factor of A Theta A^T, in precision `prec`."""

    def __init__(self, case, prec):
        T = prec
        self.prec = T
        A = self.A = case.A.astype(T)
        self.AT = np.ascontiguousarray(A.T)
        b, c, self.x, self.y, self.s, self.w, self.z = (np.asarray(v, dtype=T) for v in (case.b, case.c, case.x, case.y, case.s, case.w, case.z))
        U = self.U = case.U
        u = np.where(U, case.u, 0.0).astype(T)
        x, y, s, w, z = self.x, self.y, self.s, self.w, self.z
        self.n, self.nU = case.n, int(U.sum())
        self.aty = self.AT @ y
        self.rb = A @ x - b
        self.rc = self.aty + s - z - c
        self.ru = np.where(U, x + w - u, T(0))
        th = x / s
        th[U] = 1 / (s[U] / x[U] + z[U] / w[U])
        self.theta = th
        if T is LD:
            self.L = IO.cholesky(IO._normal_matrix(A, th))
        else:
            self.L = np.linalg.cholesky((A * th) @ A.T)

    def solve(self, r):
        if self.prec is LD:
            return IO.cholesky_solve(self.L, r)
        return np.linalg.solve(self.L.T, np.linalg.solve(self.L, r))

    def direction(self, r3, r4):
        """iteration_oracle._directions.direction, with the cached factor."""
        T, U, x, s, w, z, ru = self.prec, self.U, self.x, self.s, self.w, self.z, self.ru
        t = self.rc - r3 / x
        t[U] += (r4[U] - z[U] * ru[U]) / w[U]
        v = self.theta * t
        dy = self.solve(-self.rb - self.A @ v)
        atdy = self.AT @ dy
        dx = self.theta * atdy + v
        ds = -(r3 + s * dx) / x
        dw, dz = np.zeros(self.n, dtype=T), np.zeros(self.n, dtype=T)
        dw[U] = -ru[U] - dx[U]
        dz[U] = -(r4[U] + z[U] * dw[U]) / w[U]
        return dict(dx=dx, dy=dy, ds=ds, dw=dw, dz=dz, atdy=atdy)

    def ratios(self, d):
        rp, _, arg_p, _ = IO.ratio_test(self.x, d["dx"], self.w, d["dw"])
        rd, _, arg_d, _ = IO.ratio_test(self.s, d["ds"], self.z, d["dz"])
        return self.prec(rp), self.prec(rd), arg_p, arg_d

    def mehrotra(self, case, eta):
        """-> (corrected direction, r3c, r4c, sm, ratio_p, ratio_d, argmin_p, argmin_d, the K = 0 oracle or None)"""
        T, U, x, s, w, z = self.prec, self.U, self.x, self.s, self.w, self.z
        if T is LD:
            o = IO.iterate(case, eta)
            dxa, dsa, dwa, dza, sigma, mu = o["dxa"], o["dsa"], o["dwa"], o["dza"], o["sigma"], o["mu"]
            cor = {k: o[k] for k in ("dx", "dy", "ds", "dw", "dz", "atdy")}
        else:
            o = None
            r4 = np.zeros(self.n)
            r4[U] = w[U] * z[U]
            aff = self.direction(x * s, r4)
            aap, aad, _, _ = self.ratios(aff)
            N = T(self.n + self.nU)
            mu = (x @ s + w @ z) / N
            mu_aff = ((x + aap * aff["dx"]) @ (s + aad * aff["ds"]) + (w + aap * aff["dw"]) @ (z + aad * aff["dz"])) / N
            sigma = (mu_aff / mu) ** 3
            dxa, dsa, dwa, dza = aff["dx"], aff["ds"], aff["dw"], aff["dz"]
            cor = None
        sm = sigma * mu
        r3c = x * s + dxa * dsa - sm
        r4c = np.zeros(self.n, dtype=T)
        r4c[U] = w[U] * z[U] + dwa[U] * dza[U] - sm
        if cor is None:
            cor = self.direction(r3c, r4c)
        rp, rd, arg_p, arg_d = self.ratios(cor)
        return cor, r3c, r4c, sm, rp, rd, arg_p, arg_d, o


def _target(v, sm, T):
    t = np.minimum(np.maximum(v, T(BETA_MIN) * sm), T(BETA_MAX) * sm) - v
    return np.maximum(t, -T(BETA_MAX) * sm)


def iterate(case, K, eta=IO.ETA, prec=LD):
    """One iteration with up to K rounds -> dict:
    rounds: one dict per round that did work, in order: the candidate (dx, dy, ds, dw, dz, atdy), its complementarity terms (r3g, r4g) and those it started from (r3c, r4c),
        alpha_hat_p/d, margin, accepted, and the blocking component of each of its ratio tests (argmin_p/d: (part, column), part 1 = w / z)
    the final direction (dx, dy, ds, dw, dz, atdy), alpha_p/d, the next iterate (xn, yn, sn, wn, zn, atyn), argmin_p/d of the final
    direction, r3, r4 (its complementarity terms), mehrotra (iteration_oracle.iterate's dict; longdouble only)
    rounds_run, rounds_accepted."""
    T = prec
    B = _Base(case, T)
    cur, r3, r4, sm, rp, rd, arg_p, arg_d, o = B.mehrotra(case, eta)
    eta = T(eta)
    one = T(1)
    ap, ad = min(one, eta * rp), min(one, eta * rd)
    x, s, w, z, U = B.x, B.s, B.w, B.z, B.U
    rounds = []
    for _ in range(K):
        tp, td = min(one, ap + T(DELTA)), min(one, ad + T(DELTA))
        r3g = r3 - _target((x + tp * cur["dx"]) * (s + td * cur["ds"]), sm, T)
        r4g = np.zeros(B.n, dtype=T)
        r4g[U] = r4[U] - _target((w[U] + tp * cur["dw"][U]) * (z[U] + td * cur["dz"][U]), sm, T)
        cand = B.direction(r3g, r4g)
        hp, hd, cp, cd = B.ratios(cand)
        ahp, ahd = min(one, eta * hp), min(one, eta * hd)
        margin = ahp + ahd - ap - ad - T(GAMMA) * T(DELTA)
        ok = bool(margin >= 0)
        rounds.append(dict(cand, r3c=r3, r4c=r4, r3g=r3g, r4g=r4g, alpha_hat_p=ahp, alpha_hat_d=ahd, margin=margin, accepted=ok, argmin_p=cp, argmin_d=cd))
        if not ok:
            break
        cur, r3, r4, ap, ad, arg_p, arg_d = cand, r3g, r4g, ahp, ahd, cp, cd
    out = dict(rounds=rounds, rounds_run=len(rounds), rounds_accepted=sum(r["accepted"] for r in rounds), mehrotra=o, r3=r3, r4=r4,
               alpha_p=ap, alpha_d=ad, argmin_p=arg_p, argmin_d=arg_d, sm=sm,
               xn=x + ap * cur["dx"], yn=B.y + ad * cur["dy"], sn=s + ad * cur["ds"], wn=w + ap * cur["dw"], zn=z + ad * cur["dz"],
               atyn=B.aty + ad * cur["atdy"], rb=B.rb, rc=B.rc, ru=B.ru)
    out.update({k: cur[k] for k in ("dx", "dy", "ds", "dw", "dz", "atdy")})
    return out


def truncate(o, K, case):
    """The K-round oracle from a longdouble one computed with more rounds: the rounds are a chain, so the first K of them are the
    K-round run (K = 0: Mehrotra's step, from iteration_oracle.iterate's own dict)."""
    if K >= o["rounds_run"]:
        return o
    rounds = o["rounds"][:K]                      # all accepted (a rejected round is the last one that ran)
    m = o["mehrotra"]
    x, y, s, w, z = (np.asarray(v, dtype=LD) for v in (case.x, case.y, case.s, case.w, case.z))
    if K == 0:
        last, ap, ad = m, m["alpha_p"], m["alpha_d"]
        r3, r4 = o["rounds"][0]["r3c"], o["rounds"][0]["r4c"]
    else:
        last = rounds[-1]
        ap, ad, r3, r4 = last["alpha_hat_p"], last["alpha_hat_d"], last["r3g"], last["r4g"]
    out = dict(o, rounds=rounds, rounds_run=K, rounds_accepted=K, r3=r3, r4=r4, alpha_p=ap, alpha_d=ad,
               argmin_p=last["argmin_p"], argmin_d=last["argmin_d"],
               xn=x + ap * last["dx"], yn=y + ad * last["dy"], sn=s + ad * last["ds"], wn=w + ap * last["dw"], zn=z + ad * last["dz"],
               atyn=m["aty"] + ad * last["atdy"])
    out.update({k: last[k] for k in ("dx", "dy", "ds", "dw", "dz", "atdy")})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cells of tests/test_gpu_mcc.py.  tests/test_mcc_oracle_host.py asserts their preconditions (every accept margin at least
# 1e-6 in magnitude; a cell whose rounds 1 and 2 are both accepted; a cell with a rejected round while K leaves rounds over; a cell
# whose blocking component after a round is a w or z component), so a seed below may only be replaced by one that keeps them.
# Shapes: where the round kernels can go wrong -- one block with padding, one column in the last block, the unbounded
# instantiation over several blocks, the first grid-stride trip with and without bounds; the full-step case starts from alpha = eta.
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 65, True), (130, 257, True), (300, 513, False), (129, 16385, False), (129, 16385, True)]
SEEDS = {(5, 65, True): 2, (130, 257, True): 2, (300, 513, False): 2, (129, 16385, False): 1, (129, 16385, True): 2}
FULL_STEP = (129, 16385, 1)                                   # (m, n, seed) of iteration_oracle.full_step_case
SPARSE_DENSITY = 0.05

_cases, _oracles = {}, {}


def cell_name(m, n, bounded, sparse=False):
    return ("sparse/" if sparse else "dense/") + IO.shape_name(m, n, bounded)


def _build(name):
    if name == "full":
        return IO.full_step_case(*FULL_STEP)
    kind, shape = name.split("/")
    bounded = shape.endswith("b")
    m, n = (int(v) for v in shape.rstrip("b").split("x"))
    case = IO.interior_case(m, n, bounded, SEEDS[(m, n, bounded)])
    return IO.sparsify(case, SPARSE_DENSITY) if kind == "sparse" else case


CELLS = [cell_name(*sh) for sh in SHAPES] + [cell_name(*sh, sparse=True) for sh in SHAPES] + ["full"]


def get(name):
    """The case of a cell, built once per process.  Treat it as read-only."""
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def oracle(name, K=MAX_K):
    """The oracle of a cell with K <= MAX_K rounds (computed once with MAX_K rounds, shorter runs are its prefixes)."""
    if name not in _oracles:
        _oracles[name] = iterate(get(name), MAX_K)
    return truncate(_oracles[name], K, get(name))
