"""The conditions under which tests/test_gpu_small_free.py means something, checked without a GPU (tests/small_free_cases.py has the
cells), and the host side of the feature: the flag, the keyword, the front end's checks, the translation helper.

1. Every cell is what it claims: shape, tile count and padding rows, where its free columns sit (both sides of the 512-column stride,
   between bounded columns, the -I block of the factor form in the last rows), x = 0 and x < 0 on free columns, s != 0 there in the
   case (the seams must zero it), g > 0 and no bound there, at least one pair left, a product list within the small path's limit.
2. The reference alone stays within the condition: the longdouble one-iteration oracle is finite on every cell and its float64
   restatement agrees with it to the floor of test_gpu_iteration_edges._bound (1e-12) on every compared quantity; solve64 converges
   on every whole-solve problem within the cap the GPU test uses.
3. IPM_FLAG_SMALL_FREE is bit 8 through the header's expression and agrees with _lib; free_small is a keyword of IpmSolver, solve,
   solve_with_info and interior_sparse, off by default; solve_small_factor_qp_batch is exported with its parameter list.
4. solve_small_factor_qp_batch raises its ValueErrors, each naming the problem's index, before _lib.load() is reached; m + k = 128
   passes the host check and 129 does not.
5. factor_qp_solution is what solve_factor_qp produced before it was factored out, on recorded inputs.
"""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batches, factor_qp

import free_qp_oracle as FO
import iteration_oracle as IO
import small_free_cases as SF
import small_path_cases as SP
from test_gpu_iteration_edges import FLOOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (m, n, bounded, (tiles, padding rows), number of free columns)
SHAPES = {"1x2": (1, 2, False, (1, 15), 1), "stride/5x600": (5, 600, False, (1, 11), 4), "stride/5x600b": (5, 600, True, (1, 11), 4),
          "between/17x40b": (17, 40, True, (2, 15), None), "5x50-all-but-one": (5, 50, False, (1, 11), 49), "factor/16x40": (16, 40, False, (1, 0), 4),
          "factor/17x40": (17, 40, False, (2, 15), 4), "factor/128x300": (128, 300, False, (8, 0), 16)}


# ---- 1. structure ----------------------------------------------------------------------------------------------------------
def test_the_cells_are_the_ones_named():
    assert SF.CELLS == list(SHAPES) and SF.STRIDE == 512 and FLOOR == 1e-12
    before = dict(FO.SOLVE_PROBLEMS)
    SF.problem("50x130k10b")
    assert FO.SOLVE_PROBLEMS == before                                     # free_qp_oracle's own table is as it was


@pytest.mark.parametrize("name", SF.CELLS)
def test_cell_is_what_it_claims(name):
    m, n, bounded, tiles, nfree = SHAPES[name]
    case, g, free = SF.get(name)
    fm = FO.free_mask(free, n)
    assert case.A.shape == (m, n) and m <= 128 and SP.tiles(m) == tiles and case.bounded == bounded
    assert SP.term_count(case.A) <= SP.TERM_LIMIT
    assert nfree is None or len(free) == nfree
    assert 0 < fm.sum() < n and np.all(g[fm] > 0) and not case.U[fm].any() and np.all(case.w[fm] == 0) and np.all(case.z[fm] == 0)
    assert np.all(case.s[fm] != 0)                                          # whatever the case drew: every seam must zero it
    assert np.all(case.x[~fm] > 0) and np.all(case.s[~fm] > 0)
    if name.startswith("stride/"):
        assert list(free) == [0, SF.STRIDE - 1, SF.STRIDE, n - 1] and case.x[SF.STRIDE - 1] == 0.0 and case.x[SF.STRIDE] < 0
    if name == "between/17x40b":
        assert len(free) >= 3 and all(case.U[j - 1] and case.U[j + 1] for j in free)
        nb = int(free[1]) - 1
        assert case.w[nb] == 1e-2 and case.x[nb] + case.w[nb] == case.u[nb]
    if name == "5x50-all-but-one":
        assert np.flatnonzero(~fm).tolist() == [7] and (case.x[fm] == 0).any() and (case.x[fm] < 0).any()
    if name in SF.FACTOR:
        k = SF.FACTOR[name][2]
        assert list(free) == list(range(n - k, n)) and np.array_equal(case.A[:, n - k:], np.vstack([np.zeros((m - k, k)), -np.eye(k)]))
        assert np.all(case.A[m - k:, :n - k] != 0) and (case.x[fm] < 0).any() and (case.x[fm] > 0).any() and np.all(g[fm] == 1.0)


# ---- 2. the reference alone ------------------------------------------------------------------------------------------------
VECTORS = {"rc": "rc", "theta": "theta", "va": "va", "qa": "qa", "v": "v", "q": "q", "dxa": "dxa", "dya": "dya", "dsa": "dsa", "dx": "dx", "dy": "dy",
           "ds": "ds", "dw": "dw", "dz": "dz", "xn": "xn", "yn": "yn", "sn": "sn", "wn": "wn", "zn": "zn"}
SCALARS = ("gap", "mu", "mu_aff", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "objective", "rp_norm", "rd_norm")


@pytest.mark.parametrize("name", SF.CELLS)
def test_oracle_is_finite_and_float64_agrees(name):
    case, g, free = SF.get(name)
    o = SF.oracle(name)
    o64 = FO.iterate(case, g, free, T=np.float64)
    fm = FO.free_mask(free, case.n)
    worst = {}
    for k in VECTORS:
        assert np.all(np.isfinite(np.asarray(o[k], dtype=np.float64))), (name, k)
        worst[k] = IO.rel(np.asarray(o64[k], dtype=np.float64), o[k])
    for k in SCALARS:
        assert np.isfinite(float(o[k])), (name, k)
        worst[k] = abs(float(o64[k]) - float(o[k])) / max(abs(float(o[k])), 1e-300)
    assert np.all(o["sn"][fm] == 0) and np.all(o["ds"][fm] == 0) and np.all(o["dsa"][fm] == 0) and np.all(o["qa"][fm] == 0)
    assert 0 < float(o["alpha_p"]) <= 1 and o["alpha_p"] == o["alpha_d"] and float(o["mu"]) > 0
    print("FLOAT64 %s worst %s" % (name, max(worst.items(), key=lambda kv: kv[1])))
    assert max(worst.values()) <= FLOOR, (name, {k: v for k, v in worst.items() if v > FLOOR})


@pytest.mark.parametrize("name", SF.SOLVE_NAMES + [SF.BEYOND])
def test_float64_loop_converges_within_the_cap(name):
    A, b, c, g, F, u, xs, ys = SF.problem(name)
    r = SF.host_loop(name)
    m, n, k, seed, bounded = dict(FO.SOLVE_PROBLEMS, **SF.SOLVES, **{SF.BEYOND: SF.BEYOND_PROBLEM})[name]
    assert A.shape == (m, n) and F.shape == (n, k) and (u is not None) == bounded
    assert (m + k <= 128) == (name != SF.BEYOND) and (name != "100x300k28" or m + k == 128) and (name != SF.BEYOND or m + k == 129)
    print("LOOP64 %s iterations %d x_err %.3e" % (name, r["iterations"], r["x_err"]))
    assert r["converged"] and r["iterations"] <= SF.SOLVE_CAP - 2 and r["x_err"] <= 1e-7


# ---- 3. the flag, the keyword, the export ----------------------------------------------------------------------------------
def test_flag_value_through_the_header_expression():
    txt = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    literal = {k: int(v) for k, v in re.findall(r"\b(IPM_FLAG_[A-Z_]+)\s*=\s*(\d+)", txt)}
    shifted = dict(re.findall(r"\b(IPM_FLAG_[A-Z_]+)\s*=\s*(IPM_FLAG_[A-Z_]+)\s*<<\s*1\b", txt))
    assert shifted["IPM_FLAG_LOCKSTEP_BOUNDS"] == "IPM_FLAG_SMALL_QUADRATIC" and shifted["IPM_FLAG_SMALL_FREE"] == "IPM_FLAG_LOCKSTEP_BOUNDS"
    assert "IPM_FLAG_SMALL_FREE" not in literal                             # (the header states it by the expression, not by a literal)
    value = literal["IPM_FLAG_SMALL_QUADRATIC"] << 1 << 1
    assert value == 256 == _lib.FLAG_SMALL_FREE and _lib.FLAG_LOCKSTEP_BOUNDS == 128
    api = open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "ipm_api.hip")).read()
    assert "static_assert(IPM_FLAG_SMALL_FREE == 256" in api and "static_assert(IPM_FLAG_LOCKSTEP_BOUNDS == 128" in api
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt)              # additive: the ABI version stays


def test_signatures_and_export():
    for fn in (ipm.IpmSolver.__init__, ipm.solve, ipm.solve_with_info, ipm.interior_sparse):
        p = inspect.signature(fn).parameters
        assert p["free_small"].default is False, fn
        named = [k for k, v in p.items() if v.kind is not inspect.Parameter.VAR_KEYWORD]
        assert named[-1] == "free_small", fn                               # appended
    p = inspect.signature(ipm.solve_small_factor_qp_batch).parameters
    assert list(p) == ["problems", "tol", "max_iter", "y0", "device", "tol_gap", "ub", "regularize", "scale", "scale_passes"]
    assert (p["tol"].default, p["max_iter"].default, p["y0"].default, p["device"].default, p["tol_gap"].default, p["ub"].default,
            p["regularize"].default, p["scale"].default, p["scale_passes"].default) == (1e-8, 5000, 1.0, 0, None, None, 0.0, None, ipm.solver.SCALE_PASSES)
    assert "start" not in p and "solve_small_factor_qp_batch" in ipm.__all__
    assert "free" not in inspect.signature(ipm.solve_small_qp_batch).parameters       # the pinned front ends keep their lists
    assert inspect.signature(ipm.solve_small_batch).parameters["free"].default is None


# ---- 4. the front end's host checks ----------------------------------------------------------------------------------------
def _ok(m=20, n=40, k=3, seed=1):
    A = sparse.random(m, n, density=0.3, random_state=seed, format="csc") + sparse.eye(m, n, format="csc")
    F = np.random.default_rng(seed).standard_normal((n, k))
    return A, np.ones(m), np.ones(n), F, np.linspace(0.0, 1.0, n)


def test_small_factor_qp_batch_refuses_on_the_host(monkeypatch):
    """The host check runs before the library is loaded and before any handle exists."""
    def no_device(*a, **k):
        raise AssertionError("the library was reached before the host check refused the batch")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(factor_qp, "IpmSolver", no_device)
    ok = _ok()
    A, b, c, F, g = ok
    rng = np.random.default_rng(0)
    wide = lambda m, k: (rng.standard_normal((m, 300)), np.ones(m), np.ones(300), rng.standard_normal((300, k)), None)          # noqa: E731
    with pytest.raises(ValueError, match="problem 1 has 101 rows and 28 factors"):
        ipm.solve_small_factor_qp_batch([ok, wide(101, 28)])
    with pytest.raises(ValueError, match="problem 0 has 129 rows and 0 factors"):
        ipm.solve_small_factor_qp_batch([(rng.standard_normal((129, 300)), np.ones(129), np.ones(300), None, None), ok])
    checked = factor_qp._small_factor_qp_host_check([ok, wide(100, 28), wide(128, 0)], None)      # m + k = 128: accepted
    assert [p[0].shape[0] for p in checked] == [23, 128, 128] and checked[2][5] is None and checked[1][5].tolist() == list(range(300, 328))
    for bad in (np.nan, np.inf):
        Fb = F.copy()
        Fb[7, 1] = bad
        with pytest.raises(ValueError, match="problem 1: F must be finite"):
            ipm.solve_small_factor_qp_batch([ok, (A, b, c, Fb, g)])
    for bad in (-1.0, np.nan, np.inf):
        gb = g.copy()
        gb[7] = bad
        with pytest.raises(ValueError, match="problem 2: quad must be finite and >= 0"):
            ipm.solve_small_factor_qp_batch([ok, (A, b, c, F, None), (A, b, c, F, gb)])
        with pytest.raises(ValueError, match="problem 0: quad must be finite and >= 0"):
            ipm.solve_small_factor_qp_batch([(A, b, c, None, gb)])
    with pytest.raises(ValueError, match="problem 1: F must be n x k with n = 40 rows"):
        ipm.solve_small_factor_qp_batch([ok, (A, b, c, F[:-1], g)])
    with pytest.raises(ValueError, match="problem 1: F must be n x k"):
        ipm.solve_small_factor_qp_batch([ok, (A, b, c, np.ones(40), g)])
    with pytest.raises(ValueError, match="problem 1: quad has 39 entries, the problem has 40 columns"):
        ipm.solve_small_factor_qp_batch([ok, (A, b, c, F, g[:-1])])
    with pytest.raises(ValueError, match="problem 1: b has 19 entries, expected 20"):
        ipm.solve_small_factor_qp_batch([ok, (A, b[:-1], c, F, g)])
    with pytest.raises(ValueError, match="problem 1: A must be 2-D"):
        ipm.solve_small_factor_qp_batch([ok, (np.ones(5), b, c, F, g)])
    with pytest.raises(ValueError, match="problem 1: A has no nonzero entry"):
        ipm.solve_small_factor_qp_batch([ok, (np.zeros((20, 40)), b, c, F, g)])
    with pytest.raises(ValueError, match=r"problem 1: expected \(A, b, c, F, g\)"):
        ipm.solve_small_factor_qp_batch([ok, (A, b, c, g)])
    with pytest.raises(ValueError, match="one per problem"):
        ipm.solve_small_factor_qp_batch([ok, ok], ub=[None])
    with pytest.raises(ValueError, match="problem 1: ub must be >= 0"):
        ipm.solve_small_factor_qp_batch([ok, ok], ub=[None, -np.ones(40)])
    # the product list is counted on the AUGMENTED matrix: the k rows F^T are dense.  A alone, one entry per column: 1600 terms;
    # with k = 100 factor rows every column holds 101 entries: 1600 * 101 * 102 / 2 + 100 = 8 241 700 > 2^22
    thin = sparse.csc_matrix(np.tile(np.eye(4), (1, 400)))
    with pytest.raises(ValueError, match="problem 1: the product list of the augmented A D\\^2 A\\^T has 8241700 terms"):
        ipm.solve_small_factor_qp_batch([ok, (thin, np.ones(4), np.ones(1600), np.ones((1600, 100)), None)])
    with pytest.raises(ValueError, match="scale"):
        ipm.solve_small_factor_qp_batch([ok], scale="geometric")
    with pytest.raises(TypeError):
        ipm.solve_small_factor_qp_batch([ok], start="mehrotra")             # no such parameter: Mehrotra's start is refused for free columns
    assert factor_qp.SMALL_TERM_LIMIT == batches.SMALL_TERM_LIMIT == SP.TERM_LIMIT


def test_existing_front_ends_keep_their_refusals(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was reached")))
    A, b, c, F, g = _ok()
    with pytest.raises(ValueError, match="takes no free columns"):
        ipm.solve_small_batch([(A, b, c)], free=[3])
    with pytest.raises(TypeError):
        ipm.solve_small_qp_batch([(A, b, c, g)], free=[3])


# ---- 5. the translation helper ---------------------------------------------------------------------------------------------
def _before(xa, ya, sa, info, F, c_, g_, m, n, k):
    """The body solve_factor_qp had behind its solve_with_info call before the helper existed, restated."""
    x, y, s = xa[:n], ya[:m], sa[:n]
    Fm, xv = np.asarray(F, dtype=np.float64), x.reshape(-1)
    ftx = Fm.T @ xv
    info = dict(info)
    info["factors"], info["t"], info["y_factor"] = k, xa[n:].reshape(-1).copy(), ya[m:].reshape(-1).copy()
    info["objective_augmented"] = info["objective"]
    info["objective"] = float(c_[:n] @ xv + 0.5 * (g_[:n] * xv) @ xv + 0.5 * (ftx @ ftx))
    for key in ("w", "z"):
        if key in info:
            info[key] = info[key][:n]
    return x, y, s, info


@pytest.mark.parametrize("bounded", [False, True])
def test_translation_helper_equals_the_inline_code(bounded, monkeypatch):
    m, n, k = 7, 19, 3
    rng = np.random.default_rng(42)
    A, b, c, g, F = sparse.random(m, n, density=0.5, random_state=3, format="csc"), rng.standard_normal(m), rng.standard_normal(n), rng.uniform(0, 2, n), rng.standard_normal((n, k))
    ub = np.where(rng.random(n) < 0.5, 3.0, np.inf) if bounded else None
    A_, b_, c_, g_, u_, free = ipm.factor_qp_form(A, b, c, g, F, ub)
    xa, ya, sa = rng.standard_normal((n + k, 1)), rng.standard_normal((m + k, 1)), rng.uniform(0, 1, (n + k, 1))
    info = {"objective": 1.25, "status": 1, "iterations": 9, "quadratic_path": "one-workgroup"}
    if bounded:
        info["w"], info["z"] = rng.uniform(0, 1, (n + k, 1)), rng.uniform(0, 1, (n + k, 1))
    recorded = (xa.copy(), ya.copy(), sa.copy(), dict(info))
    want = _before(xa, ya, sa, info, F, c_, g_, m, n, k)
    got = factor_qp.factor_qp_solution(xa, ya, sa, info, F, c_, g_, m, n)
    seen = {}

    def fake(A2, b2, c2, **kw):
        seen.update(kw)
        return recorded
    monkeypatch.setattr(factor_qp, "solve_with_info", fake)
    through = ipm.solve_factor_qp(A, b, c, F, g=g, ub=ub, free_small=True, tol=1e-9)
    assert seen["free_small"] is True and seen["tol"] == 1e-9 and np.array_equal(seen["free"], free)
    for res in (got, through):
        for a, w_ in zip(res[:3], want[:3]):
            assert np.array_equal(a, w_)
        assert set(res[3]) == set(want[3])
        for key, v in want[3].items():
            assert np.array_equal(res[3][key], v) if isinstance(v, np.ndarray) else res[3][key] == v, key
    assert got[3]["factors"] == k and got[3]["objective_augmented"] == 1.25 and info["objective"] == 1.25 and "t" not in info
    assert got[0].shape == (n, 1) and got[3]["t"].shape == (k,) and (not bounded or got[3]["w"].shape == (n, 1))
