"""The conditions under which tests/test_gpu_small_qp.py means something, checked without a GPU (tests/qp_small_cases.py has the
cells), and the host side of the feature: the flag, the keyword, the new front end's checks.

1. Every cell is what it claims: shape, tile count and padding rows, the pattern of g (zero on the odd columns; the stride cell: as
   re-placed), the blockers of the stride cell's step in columns 512 (primal, a column with g > 0) and 511 (dual), and in every cell a
   relative separation of 1e-6 or more between the blocker and the runner-up in each of the four ratio tests.
2. In every cell but 1 x 2 the two ratio minima of the affine pair differ, and so do the two damped steps: the one-step rule
   (quad_step) changes the result, so a kernel that keeps the pair is caught.
3. The float64 restatement qp_oracle.iterate(..., T=np.float64) agrees with the longdouble oracle to the floor of
   test_gpu_iteration_edges._bound (1e-12) on every compared quantity.  A cell that misses it is ill-conditioned data.
4. solve_small_qp_batch raises its ValueErrors, each naming the problem's index, before a device is touched.
5. FLAG_SMALL_QUADRATIC is 64 and agrees with include/ipm_hip.h; quad_small is a keyword of IpmSolver, solve and solve_with_info and
   off by default; solve_small_batch still has no `quad` parameter.
"""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batches

import iteration_oracle as IO
import qp_oracle as Q
import qp_small_cases as QS
import small_path_cases as SP
from test_gpu_iteration_edges import FLOOR
from test_iteration_oracle_host import SEPARATION
from test_qp_oracle_host import SCALARS, VECTORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = IO.LD
SHAPES = {"tile/1x2b": (1, 2, True, (1, 15)), "tile/17x40b": (17, 40, True, (2, 15)), "tile/128x300b": (128, 300, True, (8, 0)),
          "tile/128x300": (128, 300, False, (8, 0)), "stride/20x513b": (20, 513, True, (2, 12)), "rows/24x64b": (24, 64, True, (2, 8)),
          "list/arrow": (128, 300, True, (8, 0))}


def test_the_cells_are_the_ones_named():
    assert QS.CELLS == list(SHAPES) and set(QS.CELLS) <= set(SP.BENIGN)
    assert SEPARATION == 1e-6 and FLOOR == 1e-12
    assert {QS.SOLVES[k] for k in QS.SOLVES} == {(50, 130, 5, True, True), (128, 300, 6, True, True), (17, 40, 8, True, False), (16, 40, 10, False, True)}
    before = dict(Q.SOLVE_PROBLEMS)
    QS.problem("small/17x40b")
    assert Q.SOLVE_PROBLEMS == before                                      # qp_oracle's own table is as it was


# ---- 1. structure ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QS.CELLS)
def test_cell_is_what_it_claims(name):
    m, n, bounded, tiles = SHAPES[name]
    case, g = QS.get(name)
    assert case.A.shape == (m, n) and m <= 128 and SP.tiles(m) == tiles and case.bounded == bounded
    assert SP.term_count(case.A) <= SP.TERM_LIMIT
    assert g.shape == (n,) and np.all(g >= 0) and np.all(np.isfinite(g)) and 0 < int((g > 0).sum()) < n       # LP and QP columns mix
    base = SP.get(name)
    if name != QS.STRIDE:
        assert case is base and np.array_equal(g, Q.quad_diagonal(n, QS.SEED))
        assert np.all(g[0::2] > 0) and np.all(g[1::2] == 0)
    else:       # a permutation of the LP cell's columns, and g a permutation of quad_diagonal's values that went with them
        assert sorted(map(tuple, case.A.T)) == sorted(map(tuple, base.A.T)) and np.array_equal(case.b, base.b)
        assert np.array_equal(np.sort(g), np.sort(Q.quad_diagonal(n, QS.SEED)))
        assert int((g > 0).sum()) == (n + 1) // 2
    if name == "rows/24x64b":
        assert [int(j) for j in np.flatnonzero(~(case.A != 0).any(axis=0))] == [63]              # the empty column
    if name == "list/arrow":
        nz = case.A != 0
        assert nz[:, 0].all() and [int(j) for j in np.flatnonzero(nz[0] & nz[127])] == [0] and g[0] > 0


def test_stride_cell_blockers_are_placed():
    case, g = QS.get(QS.STRIDE)
    rt = QS.ratio_tests(case, QS.oracle(QS.STRIDE))
    assert (QS.STRIDE_PRIMAL_AT, QS.STRIDE_DUAL_AT) == (512, 511) == (case.n - 1, case.n - 2)
    assert divmod(512, 512) == (1, 0) and divmod(511, 512) == (0, 511)       # (trip, thread): the second trip's first, the first trip's last
    assert rt["p"][1][1] == 512 and rt["d"][1][1] == 511, rt
    assert rt["p"][0] < 1 and rt["d"][0] < 1                                 # they really block
    assert g[512] > 0                                                        # the second trip reads a g that matters
    # (g moved with its column: the oracle of the re-placed cell is the unplaced cell's, up to summation order)
    base, g0 = SP.get(QS.STRIDE), Q.quad_diagonal(case.n, QS.SEED)
    assert not np.array_equal(g, g0)


@pytest.mark.parametrize("name", QS.CELLS)
def test_blockers_are_separated(name):
    case, g = QS.get(name)
    rt = QS.ratio_tests(case, QS.oracle(name))
    for k, (_, _, sep) in rt.items():
        assert sep >= SEPARATION, (name, k, sep)


# ---- 2. the one-step rule changes the result ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QS.CELLS)
def test_one_step_rule_matters(name):
    case, g = QS.get(name)
    o, pair = QS.oracle(name), Q.iterate(*QS.get(name), one_step=False)
    assert o["alpha_aff_p"] == o["alpha_aff_d"] == min(pair["alpha_aff_p"], pair["alpha_aff_d"])
    assert o["alpha_p"] == o["alpha_d"]
    rel = lambda a, b: float(abs(a - b) / max(a, b))          # noqa: E731
    if name == "tile/1x2b":
        return                                                # (two columns: the cell is there for nt = 1, not for the rule)
    assert rel(pair["alpha_aff_p"], pair["alpha_aff_d"]) > 1e-3, (name, pair["alpha_aff_p"], pair["alpha_aff_d"])
    assert rel(pair["alpha_p"], pair["alpha_d"]) > 1e-3, (name, pair["alpha_p"], pair["alpha_d"])
    # and it reaches the iterate: the next x (or s) of the pair rule is off by far more than any bound of the device test
    assert max(IO.rel(pair["xn"], o["xn"]), IO.rel(pair["sn"], o["sn"])) > 1e-6


# ---- 3. the oracle's own condition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QS.CELLS)
def test_float64_restatement_agrees_with_longdouble(name):
    case, g = QS.get(name)
    o, f = QS.oracle(name), Q.iterate(case, g, T=np.float64)
    errs = {k: IO.rel(f[k], o[k]) for k in VECTORS}
    errs.update({k: float(abs(LD(f[k]) - o[k]) / abs(o[k])) for k in SCALARS if k not in ("rp_norm", "rd_norm")})
    errs["rp_norm"] = IO.residual_rel(f["rp_norm"], o["rp_norm"], o["b_norm"])
    errs["rd_norm"] = IO.residual_rel(f["rd_norm"], o["rd_norm"], o["c_norm"])
    print("HOST64 %s max %.3e (%s)" % (name, max(errs.values()), max(errs, key=errs.get)))
    bad = {k: v for k, v in errs.items() if not v <= FLOOR}
    assert not bad, (name, bad)
    assert o["rp_norm"] > 1e-2 * o["b_norm"] and o["rd_norm"] > 1e-2 * o["c_norm"]       # residual_rel is the plain relative error
    # the term is in the objective and in r_c by far more than a bound
    lp = IO.iterate(case)
    assert abs(float(lp["objective"] - o["objective"])) > 1e-3 * abs(float(o["objective"]))
    assert abs(float(lp["rd_norm"] - o["rd_norm"])) > 1e-3 * float(o["rd_norm"])


@pytest.mark.parametrize("name", sorted(QS.SOLVES))
def test_float64_loop_converges_on_the_small_problems(name):
    A, b, c, g, u, xs, ys = QS.problem(name)
    r = QS.host_loop(name)
    m, n, seed, bounded, mixed = QS.SOLVES[name]
    assert A.shape == (m, n) and m <= 128 and (u is not None) == bounded and np.any(g > 0)
    print("LOOP64 %s iterations %d x_err %.3e" % (name, r["iterations"], r["x_err"]))
    assert r["converged"] and r["iterations"] <= 30 and r["x_err"] <= 1e-7


# ---- 4. the front end's host checks ------------------------------------------------------------------------------------------
def _ok(m=20, n=40, seed=1):
    A = sparse.random(m, n, density=0.3, random_state=seed, format="csc") + sparse.eye(m, n, format="csc")
    return A, np.ones(m), np.ones(n), np.linspace(0.0, 1.0, n)


def test_small_qp_batch_refuses_on_the_host(monkeypatch):
    """The host check runs before any handle exists: IpmSolver is never constructed."""
    def no_device(*a, **k):
        raise AssertionError("a handle was created before the host check refused the batch")
    monkeypatch.setattr(batches, "IpmSolver", no_device)
    ok = _ok()
    A, b, c, g = ok
    rng = np.random.default_rng(0)
    big = (rng.standard_normal((129, 300)), np.ones(129), np.ones(300), np.ones(300))
    with pytest.raises(ValueError, match="problem 1 has 129 rows"):
        ipm.solve_small_qp_batch([ok, big])
    with pytest.raises(ValueError, match="problem 0 has 129 rows"):
        ipm.solve_small_qp_batch([big, ok])
    for bad in (-1.0, np.nan, np.inf):
        gb = g.copy()
        gb[7] = bad
        with pytest.raises(ValueError, match="problem 2: quad must be finite and >= 0"):
            ipm.solve_small_qp_batch([ok, (A, b, c, None), (A, b, c, gb)])
    with pytest.raises(ValueError, match="problem 1: quad has 39 entries, the problem has 40 columns"):
        ipm.solve_small_qp_batch([ok, (A, b, c, g[:-1])])
    with pytest.raises(ValueError, match="problem 1: A must be 2-D"):
        ipm.solve_small_qp_batch([ok, (np.ones(5), b, c, g)])
    with pytest.raises(ValueError, match=r"problem 1: expected \(A, b, c, g\)"):
        ipm.solve_small_qp_batch([ok, (A, b, c)])
    with pytest.raises(ValueError, match="one per problem"):
        ipm.solve_small_qp_batch([ok, ok], ub=[None])
    with pytest.raises(ValueError, match="problem 1: ub has negative entries"):
        ipm.solve_small_qp_batch([ok, ok], ub=[None, -np.ones(40)])
    full = np.ones((128, 509))                                              # 509 * 128 * 129 / 2 = 4 202 304 terms > 2^22
    with pytest.raises(ValueError, match="problem 1: the product list of A D\\^2 A\\^T has 4202304 terms"):
        ipm.solve_small_qp_batch([ok, (full, np.ones(128), np.ones(509), np.ones(509))])
    with pytest.raises(ValueError, match="start must be"):
        ipm.solve_small_qp_batch([ok], start="warm")
    with pytest.raises(ValueError, match="scale"):
        ipm.solve_small_qp_batch([ok], scale="geometric")
    assert ipm.solve_small_qp_batch([]) == []
    assert batches.SMALL_TERM_LIMIT == SP.TERM_LIMIT


def test_front_end_signatures():
    p = inspect.signature(ipm.solve_small_qp_batch).parameters
    assert list(p) == ["problems", "tol", "max_iter", "y0", "device", "tol_gap", "ub", "regularize", "start", "scale", "scale_passes"]
    assert (p["tol"].default, p["max_iter"].default, p["y0"].default, p["start"].default) == (1e-8, 5000, 1.0, "reference")
    for absent in ("detect_infeasibility", "correctors", "refine", "dense_cols"):
        assert absent not in p
    assert "solve_small_qp_batch" in ipm.__all__
    assert "quad" not in inspect.signature(ipm.solve_small_batch).parameters           # the LP front end keeps its signature
    for fn in (ipm.IpmSolver.__init__, ipm.solve, ipm.solve_with_info):
        assert inspect.signature(fn).parameters["quad_small"].default is False


# ---- 5. the flag -------------------------------------------------------------------------------------------------------------
def test_flag_value_agrees_with_the_header():
    txt = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"\b(IPM_FLAG_[A-Z_]+)\s*=\s*(\d+)", txt)}
    assert flags["IPM_FLAG_SMALL_QUADRATIC"] == 64 == _lib.FLAG_SMALL_QUADRATIC
    assert sorted(flags.values()) == [1, 2, 4, 8, 16, 32, 64]                           # one bit each
    for name, value in flags.items():
        assert getattr(_lib, name[len("IPM_"):]) == value
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt)                           # additive: the ABI version stays
