"""Near-optimal states for the comparison of ONE iteration with the oracle of tests/iteration_oracle.py: the builders, a second
oracle solve by refinement, the error measures of this regime, and what the float64 host restatement itself loses there.  Shared by
tests/test_late_cases_host.py (CPU) and tests/test_gpu_late_iteration.py.  Test infrastructure only: a helper module, not a test.

The benign cases of iteration_oracle draw x, s, w, z ~ U(0.5, 2): theta = x/s lies in [0.25, 4].  An interior-point solver spends
its last iterations at states where theta spans 1/mu .. mu over a basic / non-basic partition.  late_case builds such a state:

    every column is AT LOWER, BASIC or (bounded only) AT UPPER; n_basic columns are basic
    per column: big ~ U(0.5, 2) and small = mu / big * U(0.5, 2)           (near the central path, not on it)
        basic:     x big,   s small            at upper (a bounded at-lower column moved, about 40 % of them):
        at lower:  x small, s big                  x big, s small, w small, z big
        every other bounded column: w big, z small                          (half the columns are bounded)
    b = A (x + mu U(-1, 1)),  c = A^T y + s - z + mu U(-1, 1),  u = x + w + mu U(-1, 1): every residual is O(mu)

Families (|B| = n_basic): nondeg |B| = m, dualdeg |B| = m + 20, primdeg |B| = m - 10 (A Theta A^T is then of rank m - 10 up to terms of
order mu^2: its condition number is about cond(B)^2 / mu^2 and float64 ends at mu = 1e-4).

What is asserted of the device (the GPU file): per (case, quantity) cell, error <= max(floor(quantity), MARGIN x H(case, quantity)).
H is the error of the float64 HOST restatement against the oracle, the maximum over three column orders (identity, reversed, one
seeded permutation): nothing but summation orders differs between them.  A cell whose three orders spread by more than STABLE, with
H above the floor, is dropped for both files: where three host orders differ by more than the square root of the margin, the
bound cannot be asserted of a fourth.  STABLE and MARGIN are refine_oracle's figures for "a different factorization and summation
order".  The host restatement is qp_oracle.newton in float64 (g = 0 for an LP, two step lengths): the one restatement of the suite
that returns every quantity a cell compares; without g it states what bounds_oracle.BoundedLP.iterate and oracle.ipm_oracle.iterate
state, with LAPACK's Cholesky.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg

import iteration_oracle as IO
import qp_oracle as QO
from refine_oracle import ORACLE_MARGIN as MARGIN, STABLE
from test_gpu_iteration_edges import HIST_SCALARS, _bound, measure as benign_measure

LD = IO.LD
LOWER, BASIC, UPPER = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------------
def sparse_pattern(m, n, density, rng):
    """A Gaussian matrix with about `density` of its entries kept, every row and every column non-empty."""
    mask = rng.random((m, n)) < density
    for j in np.flatnonzero(~mask.any(axis=0)):
        mask[rng.integers(m), j] = True
    for i in np.flatnonzero(~mask.any(axis=1)):
        mask[i, rng.integers(n)] = True
    return rng.standard_normal((m, n)) * mask


def late_case(m, n, mu, n_basic, bounded, seed, density=None, rb_scale=1.0, rc_scale=1.0, g=None):
    """-> IO.Case with .part (LOWER / BASIC / UPPER per column) and .mu_target.  density: A is sparse_pattern's, chosen BEFORE the state,
    so that b and c follow from the sparse A (IO.sparsify keeps c and would leave r_c = O(1)).  rb_scale, rc_scale: the primal (b and
    u) and dual (c) perturbations are mu times these, for the stop-test cases.  g: the diagonal of a QP, whose r_c has the term - g o x."""
    rng = np.random.default_rng([seed, m, n])
    A = rng.standard_normal((m, n)) if density is None else sparse_pattern(m, n, density, rng)
    order = rng.permutation(n)
    part = np.full(n, LOWER)
    part[order[:n_basic]] = BASIC
    U = np.zeros(n, dtype=bool)
    if bounded:
        U[rng.permutation(n)[: n // 2]] = True
        part[U & (part == LOWER) & (rng.random(n) < 0.4)] = UPPER

    def pair():
        big = rng.uniform(0.5, 2.0, n)
        return big, mu / big * rng.uniform(0.5, 2.0, n)

    big, small = pair()
    x, s = np.where(part == LOWER, small, big), np.where(part == LOWER, big, small)
    big, small = pair()
    w = np.where(U, np.where(part == UPPER, small, big), 0.0)
    z = np.where(U, np.where(part == UPPER, big, small), 0.0)
    y = rng.standard_normal(m)
    xb = x + rb_scale * mu * rng.uniform(-1.0, 1.0, n)
    c = A.T @ y + s - z - (0.0 if g is None else g * x) + rc_scale * mu * rng.uniform(-1.0, 1.0, n)
    u = np.where(U, x + w + rb_scale * mu * rng.uniform(-1.0, 1.0, n), np.inf)
    case = IO.Case(A=A, b=A @ xb, c=c, u=u, x=x, y=y, s=s, w=w, z=z, xb=xb, c_dual=False)
    case.part, case.mu_target = part, mu
    return case


def permute(case, perm):
    out = IO.permute_columns(case, perm)
    out.part, out.mu_target = case.part[perm], case.mu_target
    return out


FAMILIES = {"nondeg": (0, (1e-4, 1e-6, 1e-8)), "dualdeg": (20, (1e-4, 1e-6, 1e-8)), "primdeg": (-10, (1e-3, 1e-4))}
POINTS = [(f, mu) for f, (_, mus) in FAMILIES.items() for mu in mus]            # the eight family / mu points
# The seeds.  tests/test_late_cases_host.py asserts what they must keep: the caps on the dropped cells.  Which cells drop depends on
# float64 summation orders, so also on the BLAS build and its thread count; the three primdeg seeds below were chosen, among 1 .. 200,
# as those whose worst spread over all cells stayed lowest (2.4, 2.9, 3.2 against STABLE = 4) under 1, 2, 4, 8 and 16 BLAS threads, so
# that the family keeps a case with all its cells on any of them.  With SEED = 3 no nondeg or dualdeg case came near a cap.
SEED = 3
SEEDS = {"lock/130x300/primdeg/1e-03": 105, "dense/130x257/primdeg/1e-03": 95, "dense/130x257b/primdeg/1e-03": 6}


def name_of(kind, m, n, bounded, family, mu):
    return "%s/%s/%s/%.0e" % (kind, IO.shape_name(m, n, bounded), family, mu)


def _build(name, m, n, bounded, family, mu, density=None, **kw):
    return functools.partial(late_case, m, n, mu, m + FAMILIES[family][0], bounded, SEEDS.get(name, SEED), density=density, **kw)


# name -> builder.  The cells of tests/test_gpu_late_iteration.py, see the table there.
D130 = [name_of("dense", 130, 257, bd, f, mu) for bd in (False, True) for f, mu in POINTS]
D300 = [name_of("dense", 300, 513, True, "dualdeg", 1e-8), name_of("dense", 300, 513, True, "primdeg", 1e-3)]
D129 = name_of("dense", 129, 16385, True, "dualdeg", 1e-8)
D1000 = [name_of("dense", 1000, 2000, False, "primdeg", 1e-3), name_of("dense", 1000, 2000, True, "dualdeg", 1e-8)]
S130 = name_of("sparse", 130, 300, True, "dualdeg", 1e-6)
S60 = name_of("sparse", 60, 150, True, "dualdeg", 1e-6)
LOCK = [name_of("lock", 257, 520, False, "dualdeg", 1e-8), name_of("lock", 130, 300, False, "primdeg", 1e-3)]
QP = name_of("qp", 130, 257, True, "dualdeg", 1e-6)
DENSITY = {(130, 300): 0.05, (60, 150): 0.1, (257, 520): 0.05}
REFINEMENT_ABOVE = 600          # rows: beyond this the longdouble formation (m^2 n / 2) is replaced by the refinement solve (O(m n) a round)


def _registry():
    reg = {}
    for name in D130 + D300 + [D129] + D1000 + [S130, S60] + LOCK + [QP]:
        kind, shape, family, mu = name.split("/")
        bounded = shape.endswith("b")
        m, n = (int(v) for v in shape.rstrip("b").split("x"))
        reg[name] = _build(name, m, n, bounded, family, float(mu), density=DENSITY[(m, n)] if kind in ("sparse", "lock") else None,
                           g=QO.quad_diagonal(n, SEED) if kind == "qp" else None)
    return reg


CASES = _registry()
FAMILY_OF = {name: name.split("/")[2] for name in CASES}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name, built once per process.  Read-only."""
    return CASES[name]()


def quad_of(name):
    """The diagonal g of a QP cell (qp_oracle's rule: g > 0 on every second column, of order 1), None for an LP."""
    return CASES[name].keywords["g"]


# ---------------------------------------------------------------------------------------------------------------------------
# the second oracle solve: a float64 LAPACK Cholesky of fl(A Theta A^T), refined with longdouble residuals until stationary
# ---------------------------------------------------------------------------------------------------------------------------
class RefinementSolver:
    """solver argument of IO.iterate.  log: per solve (rounds, last relative step, stationary), stationary as
    refine_oracle.reference ends: the relative step fell below 2^-70 or stopped shrinking (max_rounds ran out: not stationary)."""

    def __init__(self, max_rounds=60):
        self.max_rounds, self.log = max_rounds, []

    def __call__(self, A, theta):
        A64, t64 = np.asarray(A, dtype=np.float64), np.asarray(theta, dtype=np.float64)
        cf = scipy.linalg.cho_factor((A64 * t64) @ A64.T, lower=True)
        AT = np.ascontiguousarray(A.T)

        def solve(r):
            y = np.asarray(scipy.linalg.cho_solve(cf, np.asarray(r, dtype=np.float64)), dtype=LD)
            last, rounds, stationary = np.inf, 0, False
            for rounds in range(1, self.max_rounds + 1):
                res = r - A @ (theta * (AT @ y))
                dlt = np.asarray(scipy.linalg.cho_solve(cf, np.asarray(res, dtype=np.float64)), dtype=LD)
                y = y + dlt
                step = float(np.sqrt(dlt @ dlt) / np.sqrt(y @ y))
                if step < 2.0 ** -70 or step >= last:
                    stationary = True
                    break
                last = step
            self.log.append((rounds, step, stationary))
            return y
        return solve


# ---------------------------------------------------------------------------------------------------------------------------
# the error measures of this regime
# ---------------------------------------------------------------------------------------------------------------------------
COMPONENTWISE = ("x", "s", "w", "z")


def componentwise(got, want):
    """max_j |got_j - want_j| / |want_j| over the support of want (w and z: the bounded set; the oracle's are exactly 0 outside)."""
    got, want = np.asarray(got, dtype=LD).ravel(), np.asarray(want, dtype=LD).ravel()
    on = want != 0
    return float(np.max(np.abs(got[on] - want[on]) / np.abs(want[on])))


def measure(quantity, got, o):
    """benign_measure, except: sigma by its ABSOLUTE error (it enters only as sigma mu beside x o s of order mu, and is 1e-20 in the
    nondeg cells); the next x, s, w, z ALSO componentwise, as quantity + ".cw" (the 2-norm cannot see their mu-sized half)."""
    base = quantity.split(".")[-1]
    if base == "sigma":
        return {quantity: float(abs(LD(got) - o["sigma"]))}
    out = benign_measure(quantity, got, o)
    if base in COMPONENTWISE:
        out[quantity + ".cw"] = componentwise(got, o[IO.oracle_key(quantity)])
    return out


def restated(case, r):
    """An iteration result r (the keys of IO.iterate, any number type) as the dict tests/test_gpu_iteration_edges.run_iteration
    returns for the device: the same quantities, taken the same way (dw and dz from the update, as the device's are)."""
    got = {"dxa": r["dxa"], "dsa": r["dsa"], "ATdya": r["atdya"], "dya": r["dya"], "aff.alpha_aff_p": r["alpha_aff_p"],
           "aff.alpha_aff_d": r["alpha_aff_d"], "aff.mu": r["mu"], "dx": r["dx"], "ds": r["ds"], "ATdy": r["atdy"], "dy": r["dy"],
           "cor.mu": r["mu"], "cor.sigma": r["sigma"], "x": r["xn"], "s": r["sn"], "ATy": r["atyn"], "y": r["yn"],
           "alpha_p": r["alpha_p"], "alpha_d": r["alpha_d"]}
    if case.bounded:
        got.update({"w": r["wn"], "z": r["zn"], "dw": (r["wn"] - case.w) / r["alpha_p"], "dz": (r["zn"] - case.z) / r["alpha_d"]})
    got.update({"hist." + k: r[k] for k in HIST_SCALARS})
    return got


def errors(case, r, o):
    """{cell name: error} of an iteration result against the oracle's, over every quantity and measure of a cell."""
    e = {}
    for q, v in restated(case, r).items():
        e.update(measure(q, v, o))
    return e


# The floor of a cell's bound.  An existing quantity: test_gpu_iteration_edges._bound.  A new measure: 100 x the largest error of the
# float64 host restatement in that measure over the benign cases IO.ITER_CASES, the construction _bound used for the device.
# tests/test_late_cases_host.py recomputes them and asserts these constants.  Measured on x86-64 with LAPACK's Cholesky, the maxima
# were: sigma (absolute) 2.9e-14, x.cw 4.1e-13, s.cw 1.3e-12 (all at dense/520x600, m close to n), w.cw 8.4e-14, z.cw 3.0e-13 (both at
# dense/400x520b).
NEW_FLOORS = {"x.cw": 4.1e-11, "s.cw": 1.3e-10, "w.cw": 8.4e-12, "z.cw": 3.0e-11, "sigma": 2.9e-12}


def floor(cell):
    parts = cell.split(".")
    if parts[-1] == "cw":
        return NEW_FLOORS[parts[-2] + ".cw"]
    if parts[-1] == "sigma":
        return NEW_FLOORS["sigma"]
    return _bound(cell)


# ---------------------------------------------------------------------------------------------------------------------------
# a case evaluated: the oracle, the host restatement in three column orders, H, the spread and the dropped cells
# ---------------------------------------------------------------------------------------------------------------------------
def host_iteration(case, g=None):
    """The float64 restatement on the case as it stands (column order included)."""
    if g is None:
        return QO.iterate(case, np.zeros(case.n), one_step=False, T=np.float64)
    return QO.iterate(case, g, T=np.float64)


def _in_order(case, g, perm):
    """host_iteration of the column-permuted case, its column vectors put back in the case's own order."""
    r = host_iteration(permute(case, perm), None if g is None else g[perm])
    out = {}
    for k, v in r.items():
        if isinstance(v, np.ndarray) and v.shape == (case.n,):
            back = np.empty_like(v)
            back[perm] = v
            v = back
        out[k] = v
    return out


def orders(n):
    return [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(n).permutation(n)]


class Evaluated:
    pass


@functools.lru_cache(maxsize=None)
def evaluate(name):
    """-> .case, .g, .o (the oracle's iteration), .solver (the RefinementSolver the oracle used, or None), .errs (three dicts, one per
    column order), .H, .spread, .dropped (set of cell names).  Computed once per process.  Read-only."""
    return evaluate_case(get(name), quad_of(name))


def evaluate_case(case, g=None):
    """evaluate of a case that is not in CASES (tests/small_path_cases.py has one); not cached."""
    ev = Evaluated()
    ev.case, ev.g = case, g
    ev.solver = RefinementSolver() if ev.case.m > REFINEMENT_ABOVE else None
    ev.o = QO.iterate(ev.case, ev.g) if ev.g is not None else IO.iterate(ev.case, solver=ev.solver)
    assert ev.case.m != ev.case.n
    ev.errs = [errors(ev.case, _in_order(ev.case, ev.g, p), ev.o) for p in orders(ev.case.n)]
    ev.H = {k: max(e[k] for e in ev.errs) for k in ev.errs[0]}
    ev.spread = {k: (ev.H[k] / min(e[k] for e in ev.errs) if min(e[k] for e in ev.errs) > 0 else np.inf) for k in ev.H}
    ev.dropped = {k for k in ev.H if ev.H[k] > floor(k) and ev.spread[k] > STABLE}
    return ev


def bound(name):
    """cell name -> what the device may reach in that cell of the case: max(floor, MARGIN x H), +inf for a dropped cell."""
    return bound_of(evaluate(name))


def bound_of(ev):
    return lambda cell: np.inf if cell in ev.dropped else max(floor(cell), MARGIN * ev.H[cell])


def basis_condition(case):
    """The 2-norm condition number of the basic columns of A (m x |B|)."""
    return float(np.linalg.cond(case.A[:, case.part == BASIC]))


# ---------------------------------------------------------------------------------------------------------------------------
# the stop decision: three states whose binding inequality of IO.converged is rp, rd and the gap in turn
# ---------------------------------------------------------------------------------------------------------------------------
STOP_MU = 1e-6
STOP_SCALES = {"rp": (1e4, 1e-3), "rd": (1e-3, 1e5), "gap": (1e-3, 1e-3)}          # binding -> (rb_scale, rc_scale)
STOP_SHAPES = {"multi": (130, 257, None), "small": (60, 150, 0.1)}                  # dense ingest; CSC of at most 128 rows


@functools.lru_cache(maxsize=None)
def stop_case(path, binding):
    m, n, density = STOP_SHAPES[path]
    rb, rc = STOP_SCALES[binding]
    return late_case(m, n, STOP_MU, m + 20, True, SEED, density=density, rb_scale=rb, rc_scale=rc)


def stop_sides(case):
    """(rp / (1 + ||(b, u_U)||), rd / (1 + ||c||), gap) in longdouble: the three left-hand sides of IO.converged.  tau, the smallest
    tolerance at which the oracle says converged, is their maximum."""
    A = case.A.astype(LD)
    b, c, x, y, s, w, z = (np.asarray(v, dtype=LD) for v in (case.b, case.c, case.x, case.y, case.s, case.w, case.z))
    U = case.U
    u = np.where(U, case.u, 0.0).astype(LD)
    rb, ru, rc = A @ x - b, np.where(U, x + w - u, LD(0)), A.T @ y + s - z - c
    return (float(np.sqrt(rb @ rb + ru @ ru) / (1 + np.sqrt(b @ b + u @ u))), float(IO.norm(rc) / (1 + IO.norm(c))), float(x @ s + w @ z))
