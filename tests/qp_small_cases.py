"""The cells of tests/test_gpu_small_qp.py: small separable QPs at the edges of the loops of csrc/small_lp.h, for the Quad variants of
the one-workgroup kernel (IPM_FLAG_SMALL_QUADRATIC).  Shared with tests/test_qp_small_cases_host.py, which asserts
without a GPU that every cell is what it claims.  Test infrastructure only: a helper module, not a test.

A cell is a cell of tests/small_path_cases.py paired with g = qp_oracle.quad_diagonal(n, SEED): zero on the odd columns, so LP and QP
columns mix in one wave.

    tile/1x2b        nt = 1
    tile/17x40b      two tiles, 15 padding rows
    tile/128x300b    eight tiles, the bounded instantiation
    tile/128x300     eight tiles, the plain instantiation
    stride/20x513b   g[j] read in the second trip of `for (j = tid; j < n; j += 512)`; column 512 has g > 0
    rows/24x64b      an empty column
    list/arrow       a dense column, entry (127, 0) of B

The blockers of an LP cell are not the QP's (theta and r_c change every direction), so the stride cell is re-placed here: its columns
are permuted, AND g WITH THEM, until the blocking column of the QP's primal ratio test of the step sits in column n - 1 = 512 and
the dual's in column 511: the first thread of the second trip and the last thread of the first.  The blockers come from
qp_oracle.iterate and iteration_oracle.ratio_test.  (The primal blocker under quad_diagonal's g is an LP column; it is made a QP
column first, see replace_stride, so that column 512 holds g > 0.)

Also here: the constructed problems of the whole solves (workloads.separable_qp at four small shapes), which qp_oracle's table of
problems holds under names of their own (small/...) while solves_registered() is open, so that test_gpu_qp.check_solve holds them to
its criteria unchanged.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import iteration_oracle as IO
import qp_oracle as Q
import small_path_cases as SP

SEED = Q.SEED
CELLS = ["tile/1x2b", "tile/17x40b", "tile/128x300b", "tile/128x300", "stride/20x513b", "rows/24x64b", "list/arrow"]
STRIDE = "stride/20x513b"
STRIDE_PRIMAL_AT, STRIDE_DUAL_AT = 512, 511


def ratio_tests(case, o):
    """The four ratio tests of one QP iteration from the oracle's directions -> {"aff_p" | "aff_d" | "p" | "d": (ratio minimum before
    min(1, .), (part, column) of the blocker, relative separation from the runner-up)}."""
    LD = IO.LD
    x, s, w, z = (np.asarray(v, dtype=LD) for v in (case.x, case.s, case.w, case.z))
    out = {}
    for key, (v, dv, vb, dvb) in {"aff_p": (x, o["dxa"], w, o["dwa"]), "aff_d": (s, o["dsa"], z, o["dza"]),
                                  "p": (x, o["dx"], w, o["dw"]), "d": (s, o["ds"], z, o["dz"])}.items():
        _, cand, arg, sep = IO.ratio_test(v, dv, vb, dvb)
        out[key] = (cand.min(), arg, sep)
    return out


def permute(case, g, perm):
    """Column j of the result is column perm[j] of the cell, and g goes with its column."""
    return IO.permute_columns(case, perm), g[perm]


def replace_stride(case, g):
    """The stride cell with the QP's blockers of the step placed: primal in column 512, then dual in column 511."""
    n = case.n
    col = ratio_tests(case, Q.iterate(case, g))["p"][1][1]
    if g[col] == 0:
        # The blocker is an LP column (a column with g > 0 has the smaller theta and moves less), and column 512 is to hold g > 0.
        # The entries of g of that column and of its left neighbour, a QP column, change places -- g alone, the columns stay --
        # and the blocker is found again: it must be the same column, now a QP column.
        g = g.copy()
        g[col], g[col - 1] = g[col - 1], g[col]
        assert g[col] > 0 and ratio_tests(case, Q.iterate(case, g))["p"][1][1] == col
    case, g = permute(case, g, SP._swap(n, col, STRIDE_PRIMAL_AT))
    col = ratio_tests(case, Q.iterate(case, g))["d"][1][1]
    assert col != STRIDE_PRIMAL_AT                      # (one column blocking both tests could not be placed twice)
    return permute(case, g, SP._swap(n, col, STRIDE_DUAL_AT))


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, g) of that cell, built once per process.  Treat both as read-only."""
    case = SP.get(name)
    g = Q.quad_diagonal(case.n, SEED)
    return replace_stride(case, g) if name == STRIDE else (case, g)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The longdouble oracle of that cell (qp_oracle.iterate), computed once per process and shared: read-only."""
    return Q.iterate(*get(name))


# ---------------------------------------------------------------------------------------------------------------------------
# whole solves: workloads.separable_qp, small enough for the one-workgroup path (qp_oracle.solve64 converges on all four)
# ---------------------------------------------------------------------------------------------------------------------------
SOLVES = {          # name -> (m, n, seed, bounded, mixed)
    "small/50x130bm": (50, 130, 5, True, True),
    "small/128x300bm": (128, 300, 6, True, True),
    "small/17x40b": (17, 40, 8, True, False),
    "small/16x40m": (16, 40, 10, False, True),
}


@contextlib.contextmanager
def solves_registered():
    """While open, qp_oracle.problem / host_loop -- and with them test_gpu_qp.check_solve, unchanged -- know the names of SOLVES.  The
    table of qp_oracle is as it was afterwards (its own names parametrize other files); what was built stays in the caches."""
    assert not set(SOLVES) & set(Q.SOLVE_PROBLEMS)
    Q.SOLVE_PROBLEMS.update(SOLVES)
    try:
        yield
    finally:
        for name in SOLVES:
            del Q.SOLVE_PROBLEMS[name]


def problem(name):
    with solves_registered():
        return Q.problem(name)


def host_loop(name):
    with solves_registered():
        return Q.host_loop(name)
