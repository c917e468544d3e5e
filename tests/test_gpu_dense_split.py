"""Dense-column split of the sparse factor on the device: sparse-factor handles (factor="sparse" forced) with
ipm_set_dense_columns, against the NumPy oracle and the np.longdouble direct solve of tests/dense_split_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, analysis, batches, workloads

import dense_split_cases as dc
import infeas_cases

pytestmark = pytest.mark.gpu

# Forward error of ipm_normal_solve on a split handle over the NumPy float64 oracle's on the same input, both against the
# np.longdouble direct solve.  MEASURED on an MI355X over the cases of test_solve_accuracy_against_the_oracle (arrowhead m = 300,
# k = 17 with d over 1e0, 1e+-1, 1e+-2; FIT1P with d = 1): see DEVICE_OVER_ORACLE_MEASURED; pinned at twice the largest ratio seen
# (summation orders differ: the device sums children and chunks in its own fixed order).
DEVICE_OVER_ORACLE_MEASURED = {("arrow", 0): 0.36, ("arrow", 1): 0.15, ("arrow", 2): 0.05, ("FIT1P", 0): 1.00}
DEVICE_OVER_ORACLE = 2.0 * max(DEVICE_OVER_ORACLE_MEASURED.values())


def lp_of(A):
    m, n = A.shape
    return A, np.asarray(A @ np.ones(n)).ravel(), np.ones(n)


def split_solver(A, cols, **kw):
    return ipm.IpmSolver(*lp_of(A), factor="sparse", dense_cols=cols, **kw)


@functools.lru_cache(maxsize=None)
def arrow(m, k):
    return dc.arrowhead(m=m, k=k, seed=k)


@functools.lru_cache(maxsize=None)
def reference(name, decades):
    """(A, cols, d, t, np.longdouble direct solve), computed once per case and shared."""
    if name == "FIT1P":
        A = dc.netlib("FIT1P")[0]
        t, ref = dc.fit1p_reference()                                       # (recorded: d = 1 only)
        assert decades == 0
        return A, analysis.dense_columns(A), np.ones(A.shape[1]), t, ref
    A, cols = arrow(300, 17)
    d = dc.spread_d(A.shape[1], decades, seed=3)
    t = np.random.default_rng(4).standard_normal(A.shape[0])
    return A, cols, d, t, dc.longdouble_solve(A, d, t)


# ------------------------------------------------------------------------------------------------------------ 1: W bitwise
@pytest.mark.parametrize("k", [1, 15, 16, 17, 64])
def test_w_is_bitwise_the_single_column_sweep(k):
    A, cols = arrow(300, k)
    m, n = A.shape
    d = dc.spread_d(n, 1, seed=5)
    t = np.ones(m)
    with split_solver(A, cols) as sv:
        assert sv.factor == "sparse" and sv.dense_split_info()["k"] == k
        sv.normal_solve(t, d)
        W, V, L = sv.debug_dense_split("W"), sv.debug_dense_split("V"), np.tril(sv.get_factor())
        assert np.array_equal(sv.debug_dense_split("cols"), cols)
        # the stock sp_fwd_kernel on every column alone, with the same L (the hook runs it: a handle with k = 1 holding only that
        # column has another L, its sparse part carries the diagonal term of ITS dense set)
        W1 = sv.debug_dense_split("W_stock")
    for j in range(k):
        assert np.array_equal(W[:, j].view(np.int64), W1[:, j].view(np.int64)), "column %d of %d" % (j, k)
    # W = L^-1 V to the accuracy of a triangular solve: gamma_m cond(L), once for the device's sweep and once for SciPy's
    Wref = solve_triangular(L, V, lower=True)
    bound = 2.0 * m * dc.EPS * np.linalg.cond(L)
    err = np.linalg.norm(W - Wref, axis=0) / np.linalg.norm(Wref, axis=0)
    print("k=%d cond(L)=%.3g bound=%.3g worst column error=%.3g" % (k, np.linalg.cond(L), bound, err.max()))
    assert err.max() <= bound


# ------------------------------------------------------------------------------------------------------------ 2: V and R
@pytest.mark.parametrize("m, k", [(300, 1), (300, 15), (300, 16), (300, 17), (300, 64), (129, 17), (257, 17), (1000, 17)])
def test_v_exact_and_r_against_the_oracle(m, k):
    A, cols = arrow(m, k)
    d = dc.spread_d(A.shape[1], 1, seed=6)
    with split_solver(A, cols) as sv:
        sv.normal_solve(np.ones(m), d)
        V, W, R = sv.debug_dense_split("V"), sv.debug_dense_split("W"), sv.debug_dense_split("R")
        info = sv.dense_split_info()
        perm = sv._perm
    assert info["k"] == k and info["k_padded"] == (k + 15) // 16 * 16 and info["row_chunks"] == (m + 255) // 256
    assert info["factorizations"] == 1 and 1 <= info["corrections"] <= 3           # the solve and its (at most two) own refinement rounds
    Vo = dc.split_parts(A, cols, d)[1]
    assert np.array_equal(V, Vo[perm])                                      # one correctly rounded sqrt, one product: exact
    assert np.array_equal(R, np.tril(R)) and (np.diag(R) >= 1.0).all()
    # the oracle's S = I + W^T W on the W the device holds: the Gram sums m terms per entry, the k x k Cholesky is backward stable
    S = np.eye(k) + W.T @ W
    bound = k * m * dc.EPS * np.linalg.norm(W) ** 2
    err = np.abs(R @ R.T - S).max()
    print("m=%d k=%d ||W||_F^2=%.3g bound=%.3g error=%.3g" % (m, k, np.linalg.norm(W) ** 2, bound, err))
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------ 3: accuracy
ACCURACY_CASES = [("arrow", 0), ("arrow", 1), ("arrow", 2), ("FIT1P", 0)]


def device_and_oracle_error(name, decades):
    A, cols, d, t, ref = reference(name, decades)
    with split_solver(A, cols) as sv:
        dev = dc.rel_err(sv.normal_solve(t, d), ref)
    return dev, dc.rel_err(dc.split_oracle(A, cols, d, t)["dy"], ref)


@pytest.mark.parametrize("name, decades", ACCURACY_CASES)
def test_solve_accuracy_against_the_oracle(name, decades):
    """Forward error of ipm_normal_solve on the split handle against the np.longdouble direct solve, at most DEVICE_OVER_ORACLE
    times the NumPy float64 oracle's on the same input.  Measured on an MI355X, device / oracle: arrowhead d = 1 0.36 (1.14e-16 /
    3.21e-16), d over 1e+-1 0.15 (1.31e-16 / 8.52e-16), d over 1e+-2 0.05 (1.12e-16 / 2.25e-15), FIT1P d = 1 1.00 (4.11e-13 /
    4.12e-13); the multiple is twice the largest, 2.0.  (The device's solve carries the split's own refinement rounds.)"""
    dev, orc = device_and_oracle_error(name, decades)
    print("%s d over 1e+-%d: device error %.3g, oracle error %.3g, ratio %.3g" % (name, decades, dev, orc, dev / orc))
    assert dev <= DEVICE_OVER_ORACLE * orc


def test_refinement_stabilises_the_split():
    """d over 1e+-4: B_s is far worse conditioned than B.  With refine=2 the split handle's error is within DEVICE_OVER_ORACLE of
    the UNSPLIT sparse handle's with refine=2 (the refinement residual is taken against the full A on both)."""
    A, cols, d, t, ref = reference("arrow", 4)
    with split_solver(A, cols, refine=2) as sv:
        split = dc.rel_err(sv.normal_solve(t, d), ref)
    with split_solver(A, cols) as sv:
        plain_split = dc.rel_err(sv.normal_solve(t, d), ref)
    with ipm.IpmSolver(*lp_of(A), factor="sparse", refine=2) as sv:
        assert sv.factor == "sparse" and sv.dense_split_info() is None
        unsplit = dc.rel_err(sv.normal_solve(t, d), ref)
    print("d over 1e+-4: split %.3g, split with refine=2 %.3g, unsplit with refine=2 %.3g" % (plain_split, split, unsplit))
    assert split <= DEVICE_OVER_ORACLE * unsplit


# ------------------------------------------------------------------------------------------------------------ 4: invariance
def test_bits_do_not_depend_on_mode_grid_or_fusion(monkeypatch):
    A, cols = arrow(300, 17)
    m, n = A.shape
    d = dc.spread_d(n, 1, seed=7)
    t = np.random.default_rng(8).standard_normal(m)

    def run():
        with split_solver(A, cols) as sv:
            sv.init_state(1.0)
            sv.iterate(3)
            out = [v.copy() for v in sv.get_state()] + [sv.normal_solve(t, d)]
            assert all(np.isfinite(v).all() for v in out)
            return out

    first = None
    for mode in ("level", "task"):
        for grid in ("1", "7", None):
            for fuse in ("0", "1"):
                monkeypatch.setenv("IPM_SP_MODE", mode)
                monkeypatch.setenv("IPM_SP_FUSE_FWD", fuse)
                if grid is None:
                    monkeypatch.delenv("IPM_SP_GRID", raising=False)
                else:
                    monkeypatch.setenv("IPM_SP_GRID", grid)
                got = run()
                first = first or got
                for a, b in zip(first, got):
                    assert np.array_equal(a.view(np.int64), b.view(np.int64)), (mode, grid, fuse)
    for a, b in zip(first, run()):                                          # and a repeated run
        assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------------------------------ 5: off means off
def test_a_cleared_set_is_the_untouched_handle():
    A, _ = arrow(300, 17)
    states = []
    for kw in ({}, {"dense_cols": []}):                                     # []: ipm_set_dense_columns(h, 0, NULL) before ipm_set_A_csc
        with ipm.IpmSolver(*lp_of(A), factor="sparse", **kw) as sv:
            sv.init_state(1.0)
            sv.iterate(10)
            states.append([v.copy() for v in sv.get_state()])
            out = (C.c_int64 * 8)()
            assert _lib.load().ipm_get_dense_split_info(sv._h, out) == 0 and out[0] == 0 and sv.dense_split_info() is None
    for a, b in zip(*states):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------------------------------ 6: whole solves
# The bare formulas do not survive a whole solve (in NumPy float64 either: near the optimum ||W||^2 passes 1 / eps and the correction
# cancels every digit); the library factors B_s + 1e-10 diag(V V^T) instead and refines every solve of a split handle against the
# full A.  Measured on an MI355X, unsplit / split iterations: block-angular 17 / 17, with correctors=1 16 / 16, with
# ub 17 / 17, FIT1P 27 / 27, SEBA 26 / 26, objectives equal to the ten digits printed.
def same_solve(split, plain):
    print("split: status %d, %d iterations, objective %.10g | unsplit: status %d, %d iterations, objective %.10g"
          % (split["status"], split["iterations"], split["objective"], plain["status"], plain["iterations"], plain["objective"]))
    assert split["status"] == plain["status"] == 1
    assert abs(split["objective"] - plain["objective"]) <= 1e-6 * abs(plain["objective"])
    assert abs(split["iterations"] - plain["iterations"]) <= 2


@functools.lru_cache(maxsize=None)
def block_lp():
    A, b, c, cols = workloads.block_angular_lp(400, 50, 8, seed=1)
    return A, b.ravel(), c.ravel(), cols


@pytest.mark.parametrize("variant", ["plain", "correctors", "ub"])
def test_whole_solve_block_angular(variant):
    A, b, c, cols = block_lp()
    kw = {}
    if variant == "correctors":
        kw["correctors"] = 1
    if variant == "ub":
        kw["ub"] = np.full(A.shape[1], np.inf)
        kw["ub"][:50] = 2.0                                                # x0 < 1.5 stays strictly feasible
    plain = ipm.solve_with_info(A, b, c, **kw)[3]
    split = ipm.solve_with_info(A, b, c, factor="sparse", dense_cols=cols, **kw)[3]
    assert plain["dense_cols"] is None and split["factor_path"] == "sparse"
    assert split["dense_cols"]["k"] == 8 and split["dense_cols"]["corrections"] >= 2 * split["iterations"]
    same_solve(split, plain)


@pytest.mark.parametrize("name", ["FIT1P", "SEBA"])
def test_whole_solve_netlib_mehrotra_start(name):
    A, b, c = dc.netlib(name)
    kw = dict(start="mehrotra", device_start=True)
    plain = ipm.solve_with_info(A, b, c, **kw)[3]
    split = ipm.solve_with_info(A, b, c, dense_cols="auto", **kw)[3]
    assert split["factor_path"] == "sparse" and split["dense_cols"]["k"] == analysis.dense_columns(A).size
    same_solve(split, plain)


def test_whole_solve_detects_unboundedness_with_a_split():
    A, b, c, cols = block_lp()
    case = infeas_cases.add_free_ray_column(A, b, c)                        # construction 3(c) on an LP with dense columns
    plain = ipm.solve_with_info(case["A"], case["b"], case["c"], detect_infeasibility=True)[3]
    split = ipm.solve_with_info(case["A"], case["b"], case["c"], detect_infeasibility=True, factor="sparse", dense_cols=cols)[3]
    assert split["dense_cols"]["k"] == 8
    assert split["status"] == plain["status"] == infeas_cases.KIND["dual_infeasible"]
    assert abs(split["iterations"] - plain["iterations"]) <= 2
    assert ipm.verify_certificate(case["A"], case["b"], case["c"], split["certificate"]) <= 1e-6


# ------------------------------------------------------------------------------------------------------------ 7: refusals
def raw_handle(m, n, flags, nnz):
    lib = _lib.load()
    opts = _lib.Options()
    lib.ipm_default_options(C.byref(opts))
    opts.flags, opts.sparse_nnz = flags, nnz
    h = C.c_void_p()
    _lib.check(None, lib.ipm_create(0, m, n, C.byref(opts), None, 0, None, C.byref(h)))
    return h


def test_refusals_of_the_c_abi():
    lib = _lib.load()
    i32 = C.POINTER(C.c_int32)

    def refused(h, cols, word):
        arr = np.asarray(cols, dtype=np.int32)
        assert lib.ipm_set_dense_columns(h, len(cols), arr.ctypes.data_as(i32)) == -1          # IPM_ERR_INVALID_ARG
        assert word in lib.ipm_last_error(h).decode(), lib.ipm_last_error(h)

    for flags, m, word in ((0, 300, "IPM_FLAG_SPARSE_FACTOR"), (_lib.FLAG_SPARSE_FACTOR, 128, "small path"),
                           (_lib.FLAG_SPARSE_FACTOR | _lib.FLAG_LOCKSTEP, 300, "lockstep")):
        h = raw_handle(m, 600, flags, 4000)
        try:
            refused(h, [1, 2], word)
            assert lib.ipm_set_dense_columns(h, 0, None) == 0               # clearing is accepted everywhere
        finally:
            lib.ipm_destroy(h)
    A, cols = arrow(300, 3)
    m, n = A.shape
    h = raw_handle(m, n, _lib.FLAG_SPARSE_FACTOR, A.nnz)
    try:
        refused(h, [0, n], "out of range")
        refused(h, [-1], "out of range")
        refused(h, [4, 7, 4], "duplicated")
        refused(h, list(range(65)), "IPM_MAX_DENSE_COLS")
        assert lib.ipm_set_dense_columns(h, -1, None) == -1
        assert lib.ipm_set_dense_columns(None, 1, np.zeros(1, dtype=np.int32).ctypes.data_as(i32)) == -1
        # every column that meets row 0: taking them out leaves row 0 of A empty
        hits_row0 = [j for j in range(n) if 0 in A.indices[A.indptr[j]:A.indptr[j + 1]]]
        assert 0 < len(hits_row0) <= 64
        arr = np.asarray(hits_row0, dtype=np.int32)
        assert lib.ipm_set_dense_columns(h, len(hits_row0), arr.ctypes.data_as(i32)) == 0
        ip, ii = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        rc = lib.ipm_set_A_csc(h, ip.ctypes.data_as(i32), ii.ctypes.data_as(i32), A.data.ctypes.data_as(C.POINTER(C.c_double)), A.nnz)
        assert rc == -1 and "empties row 0" in lib.ipm_last_error(h).decode()
        out = (C.c_int64 * 8)()
        assert lib.ipm_get_dense_split_info(h, out) == 0 and out[0] == 0
        cnt = C.c_int64(0)
        assert lib.ipm_debug_get_dense_split(h, 0, None, 0, C.byref(cnt)) == -5          # IPM_ERR_STATE: no split in place
    finally:
        lib.ipm_destroy(h)


def test_refusals_of_the_python_front_ends():
    A, cols = arrow(300, 3)
    with pytest.raises(ValueError, match="lockstep"):
        ipm.IpmSolver(*lp_of(A), lockstep=True, dense_cols=list(cols))
    for call in (lambda: batches.solve_lockstep([], dense_cols="auto"), lambda: batches.solve_small_batch([], dense_cols=[1])):
        with pytest.raises(ValueError, match="dense_cols"):
            call()
    small, scols = dc.arrowhead(m=100, k=2, block=25)
    with pytest.raises(ValueError, match="more than 128 rows"):
        ipm.IpmSolver(*lp_of(small), dense_cols=list(scols))
