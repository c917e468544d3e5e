"""The cells of tests/test_gpu_small_free.py: small QPs with free columns at the edges of the loops of csrc/small_lp.h, for the Free
variants of the one-workgroup kernel (IPM_FLAG_SMALL_FREE).  Shared with tests/test_small_free_host.py, which asserts
without a GPU that every cell and every whole-solve problem is what it claims.  Test infrastructure only: a helper module, not a test.

A cell is (case, g, free) as tests/free_qp_oracle.py holds them; every A goes to the device as CSC.

    1x2                      one barrier column and one free column (free_qp_oracle's own cell)
    stride/5x600             free columns at j = 0, 511, 512, 599: both sides of the PD_THREADS = 512 column stride and both ends;
    stride/5x600b            x = 0 on column 511 and x < 0 on column 512; plain and bounded
    between/17x40b           bounded: free columns between bounded ones, one beside a column 1e-2 from its bound
    5x50-all-but-one         every column free but one (free_qp_oracle's own cell)
    factor/16x40             the factor form [A 0; F^T -I] (factor_qp_form): the free columns' only entries are -1 in the last k rows.
    factor/17x40             16 rows: the last tile is full; 17 rows: a second tile with 15 padding rows
    factor/128x300           nt = 8, the full LDS image, 16 free columns whose -1 sit in rows 112 .. 127

The whole-solve problems (workloads.factor_qp) are registered in free_qp_oracle's table while solves_registered() is open.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import free_qp_oracle as FO
import iteration_oracle as IO
import qp_oracle as Q

SEED = FO.SEED
STRIDE = 512                        # PD_THREADS of csrc/small_lp.h: column j belongs to thread j % 512
STRIDE_FREE = [0, 511, 512, 599]
CELLS = ["1x2", "stride/5x600", "stride/5x600b", "between/17x40b", "5x50-all-but-one", "factor/16x40", "factor/17x40", "factor/128x300"]
FACTOR = {"factor/16x40": (16, 40, 4, 0.4), "factor/17x40": (17, 40, 4, 0.4), "factor/128x300": (128, 300, 16, 0.06)}      # (m, n, k, density of A)


def _stride(bounded):
    return FO._with_free(IO.interior_case(5, 600, bounded, SEED), STRIDE_FREE, x_free={511: 0.0, 512: -0.7})


def _between():
    """17 x 40 bounded, sparse: a free column between two bounded ones wherever the bounded set leaves room (every second such place),
    and the bounded left neighbour of one of them nearly AT its bound: w = 1e-2 with r_u = 0."""
    case = IO.sparsify(IO.interior_case(17, 40, True, SEED + 1), 0.4)
    U, mids = case.U, []
    for j in range(1, case.n - 1):                      # both neighbours bounded, and neither of them a free column itself
        if U[j - 1] and U[j + 1] and (not mids or mids[-1] < j - 1):
            mids.append(j)
    assert len(mids) >= 3
    case, g, free = FO._with_free(case, mids)
    nb = int(free[1]) - 1
    w, u = case.w.copy(), case.u.copy()
    w[nb] = 1e-2
    u[nb] = case.x[nb] + w[nb]
    return case.copy(w=w, u=u), g, free


def _factor(name):
    """[A 0; F^T -I] with A (m - k) x (n - k) sparse and F dense, as factor_qp_form builds it; the state of the k free columns has
    both signs, g = 1 there, and the case's s there is not 0 (every seam must zero it)."""
    m, n, k, density = FACTOR[name]
    base = IO.sparsify(IO.interior_case(m - k, n - k, False, SEED), density)
    rng = np.random.default_rng(3000 + m)
    F = rng.standard_normal((n - k, k)) / np.sqrt(n - k)
    A = np.block([[base.A, np.zeros((m - k, k))], [F.T, -np.eye(k)]])
    t = rng.standard_normal(k)
    xb = np.concatenate([base.xb, t])
    cat = lambda v, tail: np.concatenate([v, tail])          # noqa: E731
    case = IO.Case(A=A, b=A @ xb, c=cat(base.c, rng.standard_normal(k)), u=np.full(n, np.inf), x=cat(base.x, rng.standard_normal(k)),
                   y=cat(base.y, rng.standard_normal(k)), s=cat(base.s, rng.uniform(0.5, 2.0, k)), w=np.zeros(n), z=np.zeros(n), xb=xb, c_dual=False)
    g = Q.quad_diagonal(n, SEED)
    free = np.arange(n - k, n, dtype=np.int32)
    g[free] = 1.0
    return case, g, free


BUILDERS = {"1x2": lambda: FO.get("1x2"), "stride/5x600": functools.partial(_stride, False), "stride/5x600b": functools.partial(_stride, True),
            "between/17x40b": _between, "5x50-all-but-one": lambda: FO.get("5x50-all-but-one")}
BUILDERS.update({name: functools.partial(_factor, name) for name in FACTOR})


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, g, free) of that cell, built once per process: read-only."""
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The longdouble oracle of that cell (free_qp_oracle.iterate), computed once per process and shared: read-only."""
    return FO.iterate(*get(name))


# ---------------------------------------------------------------------------------------------------------------------------
# whole solves: workloads.factor_qp with m + k <= 128 (and one with m + k = 129, which must leave the small path)
# ---------------------------------------------------------------------------------------------------------------------------
SOLVES = {          # name -> (m, n, k, seed, bounded)
    "50x130k10b": (50, 130, 10, 7, True),
    "100x300k28": (100, 300, 28, 7, False),
}
SOLVE_NAMES = ["1x64k8b", "50x130k10b", "100x300k28"]          # (the first is free_qp_oracle's own)
BEYOND = "101x300k28"                                           # m + k = 129
BEYOND_PROBLEM = (101, 300, 28, 7, False)
SOLVE_CAP = 60                                                  # the iteration cap of the whole solves, on the device and in solve64


@contextlib.contextmanager
def solves_registered():
    """While open, free_qp_oracle.problem / host_loop know the names of SOLVES and BEYOND; the table is as it was afterwards."""
    extra = dict(SOLVES, **{BEYOND: BEYOND_PROBLEM})
    assert not set(extra) & set(FO.SOLVE_PROBLEMS)
    FO.SOLVE_PROBLEMS.update(extra)
    try:
        yield
    finally:
        for name in extra:
            del FO.SOLVE_PROBLEMS[name]


def problem(name):
    with solves_registered():
        return FO.problem(name)


def host_loop(name):
    with solves_registered():
        return FO.host_loop(name)
