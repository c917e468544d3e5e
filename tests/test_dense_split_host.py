"""Dense-column split of the sparse factor, host side: the NumPy oracle against an extended-precision direct
solve, the selection rule, the Netlib survey, prepare(), the ABI names and the refusals that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, analysis, batch, batches, workloads

import dense_split_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ipm_set_dense_columns", "ipm_get_dense_split_info", "ipm_debug_get_dense_split")


@pytest.mark.parametrize("k, decades", [(1, 0), (17, 0), (17, 2), (64, 1)])
def test_oracle_equals_the_direct_solve(k, decades):
    A, cols = dc.arrowhead(m=300, k=k, seed=k)
    d = dc.spread_d(A.shape[1], decades, seed=1)
    t = np.random.default_rng(2).standard_normal(300)
    ref = dc.longdouble_solve(A, d, t)
    o = dc.split_oracle(A, cols, d, t)
    bound, cond, amp = dc.oracle_bound(A, cols, d, t, ref)
    err = dc.rel_err(o["dy"], ref)
    print("k=%d decades=%d: cond(B_s)=%.3g amplification=%.3g bound=%.3g error=%.3g" % (k, decades, cond, amp, bound, err))
    assert err <= bound
    assert np.linalg.eigvalsh(o["S"]).min() >= 1.0 - 64 * dc.EPS * np.linalg.norm(o["S"], 2)      # S = I + W^T W needs no guard


def test_arrowhead_tree_is_three_levels_deep(built_lib):
    A, cols = dc.arrowhead(m=300, k=17)
    perm, info = analysis.sparse_factor_order(analysis.without_columns(A, cols))
    assert perm is not None and info["panel_height"] >= 3


def test_selection_picks_exactly_the_planted_columns():
    for k in (1, 15, 17, 64):
        A, cols = dc.arrowhead(m=300, k=k, seed=k)
        assert np.array_equal(analysis.dense_columns(A), cols)
    A, cols = workloads.block_angular_lp(400, 50, 8, seed=1)[0::3]
    assert np.array_equal(analysis.dense_columns(A), cols)


def test_selection_returns_nothing_without_dense_columns():
    A, cols = dc.arrowhead(m=300, k=3)
    assert analysis.dense_columns(analysis.without_columns(A, cols)).size == 0
    assert analysis.dense_columns(np.ones((200, 300))).size == 0            # a dense array has no sparse factor to protect


def test_selection_honours_the_cap_densest_first():
    A, cols = dc.arrowhead(m=300, k=20, seed=5)
    cnt = np.diff(A.indptr)
    got = analysis.dense_columns(A, max_cols=4)
    assert got.size == 4 and set(got) <= set(cols)
    assert cnt[got].min() >= np.sort(cnt[cols])[-4]
    assert analysis.dense_columns(A, max_cols=0).size == 0
    with pytest.raises(ValueError):
        analysis.dense_columns(A, max_cols=65)


def test_selection_refuses_to_empty_a_row():
    # two identical full columns are the only entries of row 0: one may go, the other must stay
    m = 200
    body = sparse.diags(np.ones(m), format="lil")
    body[0, 0] = 0.0
    full = sparse.csc_matrix(np.ones((m, 2)))
    A = sparse.hstack([sparse.csc_matrix(body), full], format="csc")
    A.eliminate_zeros()
    got = analysis.dense_columns(A)
    assert got.size == 1 and got[0] in (m, m + 1)
    left = analysis.without_columns(A, got)
    assert np.diff(left.tocsr().indptr).min() >= 1


@pytest.mark.parametrize("name, count", [("FIT1P", 22), ("SEBA", 14), ("ISRAEL", 22)])
def test_netlib_survey(name, count):
    A, _, _ = dc.netlib(name)
    cols = analysis.dense_columns(A)
    assert cols.size == count
    assert np.diff(analysis.without_columns(A, cols).tocsr().indptr).min() >= 1


def test_prepare_orders_rows_from_the_sparse_part(built_lib):
    A, b, c, cols = workloads.block_angular_lp(700, 50, 8, seed=3)
    plain = analysis.prepare(A, b, c)
    assert plain.dense_cols is None and plain.factor == "dense"            # the linking columns fill A A^T
    auto = analysis.prepare(A, b, c, dense_cols="auto")
    assert auto.factor == "sparse" and np.array_equal(auto.dense_cols, cols)
    forced = analysis.prepare(A, b, c, factor="sparse", dense_cols=list(cols))
    assert forced.factor == "sparse" and np.array_equal(forced.dense_cols, cols)
    with pytest.raises(ValueError, match="too dense"):                      # unsplit, the ordering gives up on the filled A A^T
        analysis.prepare(A, b, c, factor="sparse")
    sparse_already = analysis.prepare(*workloads.block_angular_lp(700, 50, 0, seed=3)[:3], dense_cols="auto")
    assert sparse_already.dense_cols is None                               # "auto" splits only where the unsplit rule gave up
    with pytest.raises(ValueError):
        analysis.prepare(A, b, c, factor="dense", dense_cols=list(cols))   # never dropped
    for bad in ([0, 0], [-1], [A.shape[1]], list(range(65)), "yes", [0.5]):
        with pytest.raises(ValueError):
            analysis.prepare(A, b, c, factor="sparse", dense_cols=bad)


def test_block_angular_workload_is_feasible_and_bounded():
    A, b, c, cols = workloads.block_angular_lp(300, 40, 5, seed=7)
    assert A.shape[0] == 300 and cols.size == 5 and b.shape == (300, 1) and c.shape == (A.shape[1], 1)
    A2 = workloads.block_angular_lp(300, 40, 5, seed=7)[0]
    assert (A != A2).nnz == 0                                              # the seed fixes it
    from scipy.optimize import linprog
    res = linprog(c.ravel(), A_eq=A, b_eq=b.ravel(), bounds=(0, None), method="highs")
    assert res.status == 0
    assert np.diff(analysis.without_columns(A, cols).tocsr().indptr).min() >= 1


def test_new_names_in_header_ctypes_and_package(built_lib):
    txt = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    lib = C.CDLL(built_lib)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+IPM_MAX_DENSE_COLS\s+64\b", txt) and _lib.MAX_DENSE_COLS == analysis.MAX_DENSE_COLS == 64
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt)
    assert "dense_columns" in ipm.__all__ and ipm.dense_columns is analysis.dense_columns
    for fn in (ipm.IpmSolver.__init__, ipm.solve, ipm.solve_with_info, ipm.interior_sparse, ipm.new_interior_sparse, batch.solve_one,
               analysis.prepare):
        p = inspect.signature(fn).parameters["dense_cols"]
        assert p.default is None                                          # off by default: no existing call changes path
    assert hasattr(ipm.IpmSolver, "dense_split_info")


def test_batch_front_ends_refuse_dense_cols():
    for call in (lambda: batches.solve_lockstep([], dense_cols="auto"),
                 lambda: batches.solve_small_batch_solvers([], dense_cols=[3]),
                 lambda: batches.solve_small_batch([], dense_cols="auto"),
                 lambda: batch.solve_shard_lockstep([], [], dense_cols="auto")):
        with pytest.raises(ValueError, match="dense_cols"):
            call()
