"""The cells of tests/test_gpu_small_path_edges.py: LPs of at most 128 rows at the edges of the loops of csrc/small_lp.h, the
one-workgroup copy of the whole interior-point iteration.  Shared with tests/test_small_path_cases_host.py, which asserts without a
GPU that every cell is what its name claims.  Test infrastructure only: a helper module, not a test.

Every cell is an iteration_oracle.Case built from a seed with that module's builders (the late cell with late_cases.late_case), and
is handed to the device as a csc_matrix: a dense ingest never takes the small path.  The cells live in a table of their own (CASES,
get): iteration_oracle's registry, and with it every existing test id, stays as it is.

    tile/     sparsify(interior_case): nt = ceil(m / 16) = 1, 2, 7, 8 tiles with 0, 1 and 15 padding rows; rows of five entries or more
    stride/   m = 20, n = 511, 512, 513, 1025: the primal blocker of the step in column n - 1 (a bounded one), the dual blocker in
              column 512 (n = 1025), 511 (n = 513, see stride_dual_at) or 0: the ends of the first trip of
              `for (j = tid; j < n; j += 512)` and the start of the next
    rows/     24 x 64, row i of exactly (i % 12) + 1 entries: every split of the 4-lanes-per-row sums; column 63 without an entry
    list/     m = 128: arrow (a dense column 0, entry (127, 0) of B fed by it alone), full508 and full509 (dense 128 x 508 / 509: the
              product list of 4 194 048 terms is the last that fits the rule terms <= 2^22, the one of 4 202 304 the first that does not)
    detect/   the benign 17 x 40 and 128 x 300 cells for a handle with the infeasibility tests, and the states at which a test fires
              (iteration_oracle.primal_fire_case / dual_fire_case) with the attaining column or row in the last place
    late/     late_cases' nondeg family at mu = 1e-6, sparse, 128 x 300: eight tiles where late_cases' 60 x 150 has four
    delayed/  (DELAYED, delayed_fire; not in CASES) a cell and the tolerances under which a test of the infeasibility tests fires
              first at the stop test of iteration K >= 1: the sums and maxima the launch must have reset in between
"""
from __future__ import annotations

import functools

import numpy as np

import iteration_oracle as IO
import late_cases as LC

TERM_LIMIT = 1 << 22            # ipm_set_A_csc: a product list of more terms leaves the small path (host_sparse_setup.h)
MIN_ROW = 5                     # tile/: entries per row, at least (or n where n is smaller)

# (m, n, bounded) -> (seed, density).  A seed may only be replaced by one that keeps what tests/test_small_path_cases_host.py asserts.
TILE = {(1, 2): (2, 1.0), (15, 40): (2, 0.4), (16, 40): (2, 0.4), (17, 40): (2, 0.4), (112, 300): (2, 0.06), (113, 300): (2, 0.06),
        (127, 300): (2, 0.06), (128, 300): (2, 0.06)}
TILE_UNBOUNDED = [(16, 40), (128, 300)]
STRIDE_M, STRIDE_N, STRIDE_DENSITY = 20, (511, 512, 513, 1025), 0.3
STRIDE_SEED = {511: 2, 512: 2, 513: 2, 1025: 2}
ROWS_M, ROWS_N, ROWS_SEED = 24, 64, 2
LIST_M, ARROW_N, ARROW_SEED, FULL_SEED = 128, 300, 2, 2
LATE = LC.name_of("sparse", 128, 300, True, "nondeg", 1e-6)
LATE_DENSITY = 0.05


def tiles(m):
    """(nt, padding rows) of the LDS image of B: nt = ceil(m / 16) tiles of 16 rows."""
    nt = -(-m // 16)
    return nt, 16 * nt - m


def term_count(A):
    """The terms of the product list of A diag(d) A^T: a column of c entries feeds c (c + 1) / 2 lower entries."""
    c = (np.asarray(A) != 0).sum(axis=0).astype(np.int64)
    return int((c * (c + 1) // 2).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------------
def tile_case(m, n, bounded=True):
    seed, density = TILE[(m, n)]
    case = IO.sparsify(IO.interior_case(m, n, True, seed), density)
    return case if bounded else case.without_bounds()


def stride_case(n):
    """The blockers of the step placed (IO.place); the seed is one whose primal blocker is a bounded column (it lands in n - 1)."""
    case = IO.sparsify(IO.interior_case(STRIDE_M, n, True, STRIDE_SEED[n]), STRIDE_DENSITY)
    return IO.place(case, primal_at=n - 1, dual_at=stride_dual_at(n))


def stride_dual_at(n):
    """Column 512, the first of the second trip, where there is one beside column n - 1; else column 0.  At n = 513 column 512 IS
    column n - 1 and holds the primal blocker (no seed of 1 .. 4000 has one column blocking both ratio tests): the dual blocker
    takes column 511 there, the last thread of the first trip."""
    return 512 if n > 513 else 511 if n == 513 else 0


def rows_case(bounded):
    """Row i: one entry ~ U(1, 2) in column i and i % 12 entries ~ N(0, 1) in columns 24 .. 62, taken in turn from a shuffled cycle
    of those 39 columns (so each of them is used, and no row uses one twice); column 63 stays empty.  The first 24 columns are a
    diagonal block: the rows are independent.  The state is interior_case's; the bounded set is 31 of the first 63 columns and column 63."""
    rng = np.random.default_rng(ROWS_SEED)
    m, n = ROWS_M, ROWS_N
    A = np.zeros((m, n))
    cycle, at = 24 + rng.permutation(39), 0
    for i in range(m):
        A[i, i] = rng.uniform(1.0, 2.0)
        for _ in range(i % 12):
            A[i, cycle[at % 39]] = rng.standard_normal()
            at += 1
    x, s = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    y, xb, c = rng.standard_normal(m), rng.uniform(0.5, 2.0, n), rng.standard_normal(n)
    u, w, z = np.full(n, np.inf), np.zeros(n), np.zeros(n)
    if bounded:
        cols = np.sort(np.append(rng.permutation(n - 1)[: n // 2 - 1], n - 1))
        w[cols], z[cols] = rng.uniform(0.5, 2.0, cols.size), rng.uniform(0.5, 2.0, cols.size)
        u[cols] = x[cols] + w[cols] + rng.uniform(-0.3, 0.3, cols.size)
    return IO.Case(A=A, b=A @ xb, c=c, u=u, x=x, y=y, s=s, w=w, z=z, xb=xb, c_dual=False)


def arrow_case():
    """128 x 300: column 0 dense; column j = 1 .. 128 holds rows j - 1 and (j + 1) % 128 (with j % 128, column 128 would hold rows 127
    and 0 and feed entry (127, 0) of B beside column 0); every other column two random rows, never the pair (0, 127)."""
    rng = np.random.default_rng(ARROW_SEED)
    m, n = LIST_M, ARROW_N
    base = IO.interior_case(m, n, True, ARROW_SEED)
    mask = np.zeros((m, n), dtype=bool)
    mask[:, 0] = True
    for j in range(1, m + 1):
        mask[j - 1, j] = mask[(j + 1) % m, j] = True
    for j in range(m + 1, n):
        while True:
            r = rng.choice(m, 2, replace=False)
            if set(r.tolist()) != {0, m - 1}:
                break
        mask[r, j] = True
    A = base.A * mask
    return base.copy(A=A, b=A @ base.xb)


def full_case(n):
    return IO.interior_case(LIST_M, n, True, FULL_SEED)


def _swap(n, i, j):
    perm = np.arange(n)
    perm[i], perm[j] = perm[j], perm[i]
    return perm


def fire_case(base, kind):
    """kind: "primal" (the column attaining max (A^T y - z)_+ last), "dual/row" (the row attaining ||A x||_inf last), "dual/xu" (A
    scaled so that max x_U decides, that column last)."""
    if kind == "primal":
        f = IO.primal_fire_case(base)
        return IO.permute_columns(f, _swap(f.n, IO.infeasibility(f)["col_p"], f.n - 1))
    if kind == "dual/row":
        f = IO.dual_fire_case(base)
        return IO.permute_rows(f, _swap(f.m, IO.infeasibility(f)["row_d"], f.m - 1))
    f = IO.dual_fire_case(base, xu_wins=True)
    return IO.permute_columns(f, _swap(f.n, IO.infeasibility(f)["col_xu"], f.n - 1))


def late_case():
    m, n = 128, 300
    return LC.late_case(m, n, 1e-6, m + LC.FAMILIES["nondeg"][0], True, LC.SEED, density=LATE_DENSITY)


# ---------------------------------------------------------------------------------------------------------------------------
# the table: name -> builder
# ---------------------------------------------------------------------------------------------------------------------------
def _registry():
    reg = {}
    for (m, n) in TILE:
        reg["tile/" + IO.shape_name(m, n, True)] = functools.partial(tile_case, m, n)
    for (m, n) in TILE_UNBOUNDED:
        reg["tile/" + IO.shape_name(m, n, False)] = functools.partial(tile_case, m, n, False)
    for n in STRIDE_N:
        reg["stride/" + IO.shape_name(STRIDE_M, n, True)] = functools.partial(stride_case, n)
    for bd in (True, False):
        reg["rows/" + IO.shape_name(ROWS_M, ROWS_N, bd)] = functools.partial(rows_case, bd)
    reg["list/arrow"] = arrow_case
    reg["list/full508"] = functools.partial(full_case, 508)
    reg["list/full509"] = functools.partial(full_case, 509)
    # detect/: the benign cells are the tile cells (17 x 40 without bounds: the bounded cell's A and state)
    reg["detect/17x40b"] = lambda: get("tile/17x40b")
    reg["detect/17x40"] = lambda: get("tile/17x40b").without_bounds()
    reg["detect/128x300b"] = lambda: get("tile/128x300b")
    reg["detect/128x300"] = lambda: get("tile/128x300")
    for base, kinds in (("tile/17x40b", ("primal", "dual/row", "dual/xu")), ("tile/16x40", ("primal", "dual/row")),
                        ("stride/20x513b", ("primal", "dual/row", "dual/xu"))):
        for kind in kinds:          # detect/fire/primal/<shape>/col, detect/fire/dual/<shape>/row, detect/fire/dual/<shape>/xu
            test, where = (kind + "/col").split("/")[:2]
            reg["detect/fire/%s/%s/%s" % (test, base.split("/")[1], where)] = lambda base=base, kind=kind: fire_case(get(base), kind)
    reg["late/" + LATE] = late_case
    return reg


CASES = _registry()
FIRE = [nm for nm in CASES if nm.startswith("detect/fire/")]
DETECT_BENIGN = [nm for nm in CASES if nm.startswith("detect/") and nm not in FIRE]
BENIGN = [nm for nm in CASES if nm.startswith(("tile/", "stride/", "rows/", "list/"))]
LATE_NAME = "late/" + LATE


def fire_kind(name):
    """"primal", "dual/row" or "dual/xu" of a detect/fire/ cell."""
    _, _, test, _, where = name.split("/")
    return "primal" if test == "primal" else "dual/" + where


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name, built once per process; its oracle (IO.iterate(case)) is cached on it.  Treat both as read-only."""
    return CASES[name]()


# ---------------------------------------------------------------------------------------------------------------------------
# a test that fires AFTER K >= 1 iterations of one launch: what the sums and maxima of the tests carry from one stop test to the next
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (the cell whose data and state the solve starts from, the test that is to fire, the iteration K at whose stop test)
DELAYED = {"delayed/primal/17x40b": ("detect/fire/dual/17x40b/xu", "primal", 3),       # beta turns positive there: duz and dmaty
           "delayed/dual/20x513b/xu": ("detect/fire/dual/20x513b/xu", "dual", 2),       # max x_U is larger at k = 1 than at k = 2: dmxu
           "delayed/dual/128x300": ("tile/128x300", "dual", 1)}                         # the kernel without bounds
DELAYED_MARGIN = 1.5            # the ratio at K is at most 1 / 1.5 of every earlier one; the tolerance sits sqrt(1.5) from both sides


def fire_ratios(case):
    """(vp / beta, vd / gamma) of a state, +inf where beta (gamma) is not positive: a test fires when its ratio is <= its tolerance."""
    q = IO.infeasibility(case)
    return (float(q["vp"] / q["beta"]) if q["beta"] > 0 else np.inf, float(q["vd"] / q["gamma"]) if q["gamma"] > 0 else np.inf)


@functools.lru_cache(maxsize=None)
def delayed_fire(name):
    """-> dict(case, kind, K, tol = (eps_p, eps_d), ratios, states): the oracle's trajectory from the cell's state (each next state
    rounded to float64, as the device holds it) up to iteration K, the ratios of both tests at its K + 1 stop tests, and the
    tolerances under which the named test fires first at the last of them: sqrt(DELAYED_MARGIN) above its ratio there, and at most
    half of anything the other test reaches.  tests/test_small_path_cases_host.py asserts that the earlier ratios stay
    sqrt(DELAYED_MARGIN) above the tolerance."""
    base, kind, K = DELAYED[name]
    which = 0 if kind == "primal" else 1
    states = [get(base)]
    for _ in range(K):
        o = IO.iterate(states[-1])
        states.append(states[-1].copy(**{v: np.asarray(o[v + "n"], dtype=np.float64) for v in "xyswz"}))
    ratios = [fire_ratios(at) for at in states]
    tol = [min(1e-8, 0.5 * min(r[1 - which] for r in ratios))] * 2
    tol[which] = float(np.sqrt(DELAYED_MARGIN)) * ratios[K][which]
    return dict(case=states[0], kind=kind, K=K, tol=tuple(tol), ratios=ratios, states=states)


@functools.lru_cache(maxsize=None)
def late_evaluated():
    """late_cases.evaluate_case of the late cell: the oracle, the float64 host error H in three column orders, the dropped cells."""
    return LC.evaluate_case(get(LATE_NAME))
