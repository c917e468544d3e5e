"""Infeasibility detection for quadratic problems (IPM_FLAG_DETECT_QUADRATIC, detect_qp=True) on the CPU, before
tests/test_gpu_qp_detect.py holds the device to the same cases:

  * every construction of tests/qp_infeas_cases.py carries what it claims: its exact certificate verifies to 1e-12 with
    verify_certificate's new arguments, an unbounded one has a feasible point x0 next to its ray (feasible + ray => unbounded);
  * verify_certificate REJECTS, with a violation far above the 1e-8 of the tests, an LP ray whose support meets g > 0 or has
    F^T x^ != 0, and a y whose A^T y is negative on a free column; with the new arguments at their defaults it returns what it did;
  * the float64 host loop (free_qp_oracle.newton plus the two tests) ends in the expected kind at the recorded iteration on every
    positive case, with a certificate that verifies; it converges on the negative ones without a test ever firing; with g = 0 and no
    free column it gives what infeas_cases.oracle_detection gives;
  * every ValueError of the Python front ends, before any device is touched; the flag's value in the ABI.

Bounds.  1e-12 on a constructed certificate: its entries are O(1) sums of <= 90 (130 x 300: 300) products rounded once, ~n eps = 7e-14
at most (observed <= 7.2e-15).  The loop's certificate: the test fired at eps = 1e-8 on the same quantities verify_certificate
recomputes, so 1e-8 plus rounding; mapped back to the original factor-model problem |F^T x^| <= |F^T x^ - t^| + |t^| <= 2 eps: 2e-8 is
asserted for both (observed <= 9.5e-9)."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batch, batches, factor_qp, handle

import free_qp_oracle as FO
import infeas_cases as IC
import qp_infeas_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = ipm.verify_certificate


def _verify(P, cert):
    return V(P["A"], P["b"], P["c"], cert, ub=P["ub"], g=P["g"], free=P["free"])


# ---- the constructions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QC.POSITIVE)
def test_construction_carries_its_certificate(name):
    P = QC.get(name)
    assert P["kind"] == QC.CASES[name][1]
    if P["cert"] is None:                                  # one-curved-ray-column: the ray is the loop's own
        assert name == "one-curved-ray-column"
        return
    assert P["cert"]["kind"] == P["kind"]
    v = _verify(P, P["cert"])
    print("EXACT %s %.3e" % (name, v))
    assert v <= 1e-12
    if P["kind"] == "dual_infeasible":                     # feasible + ray => unbounded
        x0, ub = P["x0"], np.full(len(P["c"]), np.inf) if P["ub"] is None else P["ub"]
        U = np.isfinite(ub)
        fm = np.zeros(len(x0), dtype=bool)
        if P["free"] is not None:
            fm[P["free"]] = True
        assert np.max(np.abs(P["A"] @ x0 - P["b"])) <= 1e-12 * max(1.0, np.max(np.abs(P["b"])))
        assert np.all(x0[~fm] >= 0) and np.all(x0[U] <= ub[U])
        d = P["cert"]["x"]
        assert P["c"] @ d < 0 and np.all(P["g"] * d == 0) and np.all(d[U] == 0)     # the objective falls linearly along it: no curvature on its support
    if "orig" in P:                                        # the same certificate against the ORIGINAL factor-model problem
        O = P["orig"]
        vo = V(O["A"], O["b"], O["c"], O["cert"], ub=O["ub"], g=O["g"], F=P["F"])
        print("EXACT-ORIGINAL %s %.3e" % (name, vo))
        assert vo <= 1e-12


def test_large_case_is_unbounded_by_construction():
    P = QC.get("large-dense")
    assert P["A"].shape == (21 * 128, 42 * 128)
    assert _verify(P, P["cert"]) <= 1e-12
    assert np.all(P["x0"] > 0) and np.array_equal(P["A"] @ P["x0"], P["b"])
    assert np.all(P["g"] * P["cert"]["x"] == 0) and (P["g"] > 0).sum() == 64


def test_verify_certificate_rejects_what_the_curvature_forbids():
    # 1. an LP ray whose support meets g > 0: exact for the LP, far from one for the QP
    P = QC.get("sep-dual/0")
    d = P["cert"]["x"]
    assert V(P["A"], P["b"], P["c"], P["cert"]) <= 1e-12
    g = np.zeros_like(d)
    g[int(np.argmax(d))] = 1.0
    assert V(P["A"], P["b"], P["c"], P["cert"], g=g) == pytest.approx(np.max(d), rel=1e-12) and np.max(d) >= 0.5
    # 2. ... or has F^T x^ != 0
    F = np.ones((len(d), 1))
    assert V(P["A"], P["b"], P["c"], P["cert"], F=F) == pytest.approx(d.sum(), rel=1e-12) and d.sum() >= 0.5
    Q = QC.get("factor-dual/0")
    O = Q["orig"]
    assert V(O["A"], O["b"], O["c"], O["cert"], ub=O["ub"], g=O["g"], F=Q["F"]) <= 1e-12
    assert V(O["A"], O["b"], O["c"], dict(O["cert"], t=np.ones(6)), ub=O["ub"], g=O["g"], F=Q["F"]) == pytest.approx(1.0, rel=1e-9)      # a t that is not F^T x^
    # 3. a y whose A^T y is NEGATIVE on a free column: fine for a column with s >= 0, a violation for a free one
    R = QC.get("sep-primal/0")
    aty = R["A"].T @ R["cert"]["y"]
    j = int(np.argmin(aty))
    assert aty[j] <= -0.1 and V(R["A"], R["b"], R["c"], R["cert"]) == 0.0
    assert V(R["A"], R["b"], R["c"], R["cert"], free=[j]) == pytest.approx(-aty[j], rel=1e-12)
    mask = np.zeros(len(aty), dtype=bool)
    mask[j] = True
    assert V(R["A"], R["b"], R["c"], R["cert"], free=mask) == V(R["A"], R["b"], R["c"], R["cert"], free=[j])
    # a nonzero multiplier of a factor row is one too
    T = QC.get("factor-primal/0")
    O = T["orig"]
    bad = dict(O["cert"], y_factor=np.full(6, 0.25))
    assert V(O["A"], O["b"], O["c"], bad, g=O["g"], F=T["F"]) >= 0.25 * (1 - 1e-12)
    # a free column lifts the sign constraint of a ray there
    x = d.copy()
    x[0] = -1e-3
    assert V(P["A"], P["b"], P["c"], dict(kind="dual_infeasible", x=x)) >= 1e-3 * 0.5
    assert V(P["A"][:, 1:], P["b"], P["c"][1:], dict(kind="dual_infeasible", x=x[1:])) <= 1e-12       # (column 0 of A times 0: nothing else moved)


@pytest.mark.parametrize("name", sorted(IC.small_instances()))
def test_verify_certificate_defaults_return_what_they_did(name):
    """The LP instances with their own certificates: g = None, free = None, F = None, and the explicit neutral values (g = 0, an empty
    free set) give the identical float."""
    P = IC.small_instances()[name]()
    A = P["A"]
    v0 = V(A, P["b"], P["c"], P["cert"], ub=P["ub"])
    n = len(P["c"])
    assert v0 == V(A, P["b"], P["c"], P["cert"], P["ub"], None, None, None)
    assert v0 == V(A, P["b"], P["c"], P["cert"], ub=P["ub"], g=np.zeros(n), free=[]) == V(A, P["b"], P["c"], P["cert"], ub=P["ub"], free=np.zeros(n, dtype=bool))
    p = inspect.signature(V).parameters
    assert list(p) == ["A", "b", "c", "cert", "ub", "g", "free", "F"] and all(p[k].default is None for k in ("ub", "g", "free", "F"))


# ---- the float64 host loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QC.POSITIVE)
def test_host_loop_detects_the_expected_kind(name):
    P, r = QC.get(name), QC.host(name)
    _, kind, k = QC.CASES[name]
    print("LOOP %s %s k=%d violation %.3e" % (name, r["kind"], r["k"], r["cert"]["violation"] if r["cert"] else np.nan))
    assert r["kind"] == kind and r["fired"] and r["k"] == k
    assert r["cert"]["k"] == k and r["cert"]["violation"] <= QC.EPS
    assert _verify(P, r["cert"]) <= 2e-8
    if "orig" in P:                                        # mapped back as solve_factor_qp maps it
        O, F = P["orig"], P["F"]
        m, n = O["A"].shape
        c = r["cert"]
        mapped = dict(kind=c["kind"], y=c["y"][:m], y_factor=c["y"][m:], z=c["z"][:n], x=c["x"][:n], t=c["x"][n:])
        assert V(O["A"], O["b"], O["c"], mapped, ub=O["ub"], g=O["g"], F=F) <= 2e-8


@pytest.mark.parametrize("name", QC.NEGATIVE)
def test_host_loop_converges_on_the_negative_cases(name):
    r = QC.host(name)
    print("LOOP %s %s k=%d" % (name, r["kind"], r["k"]))
    assert r["kind"] == "converged" and not r["fired"] and r["k"] == QC.CASES[name][2]


def test_one_curved_column_does_not_bound_the_problem():
    """the recession cone has other rays; the loop finds one whose support avoids the curved column."""
    P, r = QC.get("one-curved-ray-column"), QC.host("one-curved-ray-column")
    j = int(np.flatnonzero(P["g"])[0])
    assert r["kind"] == "dual_infeasible" and r["cert"]["x"][j] <= QC.EPS and np.max(r["cert"]["x"]) > 1e-3


@pytest.mark.parametrize("name", ["primal_dense", "dual_dense"])
def test_host_loop_with_no_term_is_the_lp_oracle(name):
    P = IC.small_instances()[name]()
    k, kind = IC.oracle_detection(P["A"], P["b"], P["c"])
    r = QC.detect_loop(P["A"], P["b"], P["c"], np.zeros(len(P["c"])))
    assert (r["k"], r["kind"]) == (k, kind) and kind == P["kind"]


# ---- the cells of the one-stop-test comparisons -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(QC.EDGE))
def test_edge_cells_fire_at_tolerance_one_half(name):
    """A constructed state: its own test fires at 0.5 with a factor 2 to spare, the other one is silent, and the quantity the cell is
    named after decides (asserted inside the builders too)."""
    case, g, free = QC.edge(name)
    kind = QC.EDGE[name][1]
    rp, rd = QC.ratios(case, g, free)
    q = QC.quantities(case, g, free)
    if kind == "dual":
        assert rd <= 0.25 and not rp <= 0.5 and q["vd"] == q["gx_max"]
    else:
        assert rp <= 0.25 and q["vp"] == q["free_max"] and not (rd <= 0.5 and not rp <= 0.5)
    if name.startswith("curv/") and "barrier" not in name:           # the curvature cells fire first at iteration 1 (.. 3) as well
        for K in ((1,) if "1x2" in name else (1, 2, 3)):
            d = QC.delayed(name, K)
            assert d is not None and all(r[1] >= d["tol"][1] * np.sqrt(QC.DELAYED_MARGIN) * (1 - 1e-12) for r in d["ratios"][:K]) and d["ratios"][K][1] < d["tol"][1]


@pytest.mark.parametrize("name", sorted(QC.PRIMAL_DELAYED))
def test_primal_delayed_cells(name):
    """The builder's own assertions (the column, the sign, the margins) hold, and the earlier ratios stay sqrt(margin) above the tolerance."""
    d = QC.primal_delayed(name)
    K = d["K"]
    assert K == QC.PRIMAL_DELAYED[name][6] and d["ratios"][K][0] < d["tol"][0]
    assert all(r[0] >= d["tol"][0] * np.sqrt(QC.DELAYED_MARGIN) * (1 - 1e-12) for r in d["ratios"][:K])
    assert all(not r[1] <= d["tol"][1] for r in d["ratios"])
    fm = FO.free_mask(d["free"], d["case"].n)
    assert fm.sum() == 3 and fm[QC.PRIMAL_DELAYED[name][4]]


# ---- the flag and the keyword --------------------------------------------------------------------------------------------------
def test_flag_value_through_the_header_expression():
    txt = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    literal = {k: int(v) for k, v in re.findall(r"\b(IPM_FLAG_[A-Z_]+)\s*=\s*(\d+)", txt)}
    shifted = dict(re.findall(r"\b(IPM_FLAG_[A-Z_]+)\s*=\s*(IPM_FLAG_[A-Z_]+)\s*<<\s*1\b", txt))
    assert shifted["IPM_FLAG_DETECT_QUADRATIC"] == "IPM_FLAG_SMALL_FREE" and "IPM_FLAG_DETECT_QUADRATIC" not in literal
    assert literal["IPM_FLAG_SMALL_QUADRATIC"] << 3 == 512 == _lib.FLAG_DETECT_QUADRATIC
    assert all(v & 512 == 0 for v in literal.values()) and _lib.FLAG_SMALL_FREE == 256
    api = open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "ipm_api.hip")).read()
    assert "static_assert(IPM_FLAG_DETECT_QUADRATIC == 512" in api
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt) and _lib.ABI_VERSION == 4              # additive: the ABI version stays


def test_signatures_and_export():
    for fn in (ipm.IpmSolver.__init__, ipm.solve, ipm.solve_with_info, ipm.interior_sparse, batches.solve_lockstep, batch.solve_shard_lockstep):
        assert inspect.signature(fn).parameters["detect_qp"].default is False, fn
    # the pinned parameter lists keep their lists; the option lives on a sibling
    for plain, sib in ((ipm.solve_small_qp_batch, ipm.solve_small_qp_batch_detect), (ipm.solve_small_factor_qp_batch, ipm.solve_small_factor_qp_batch_detect)):
        p, q = inspect.signature(plain).parameters, inspect.signature(sib).parameters
        assert "detect_qp" not in p and list(q) == list(p) + ["infeasibility_tol"] and q["infeasibility_tol"].default == (1e-8, 1e-8)
        assert all(q[k].default == p[k].default for k in p)
        assert sib.__name__ in ipm.__all__


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached before the host check refused the call")
    monkeypatch.setattr(_lib, "load", boom)


def test_value_errors_before_any_device(monkeypatch):
    _no_device(monkeypatch)
    A, b, c = sparse.csc_matrix(np.eye(3)), np.ones(3), np.ones(3)
    g = np.array([1.0, 0.0, 0.0])
    for quad in (None, np.zeros(3)):                       # detect_qp without a quadratic term
        with pytest.raises(ValueError, match="detect_qp=True without a quadratic term"):
            ipm.IpmSolver(A, b, c, quad=quad, detect_qp=True)
        with pytest.raises(ValueError, match="detect_qp=True without a quadratic term"):
            ipm.solve_with_info(A, b, c, quad=quad, detect_qp=True)
        with pytest.raises(ValueError, match="detect_qp=True without a quadratic term"):
            ipm.solve(A, b, c, quad=quad, detect_qp=True)
        with pytest.raises(ValueError, match="detect_qp=True without a quadratic term"):
            ipm.interior_sparse(A, b, c, quad=quad, detect_qp=True)
    with pytest.raises(ValueError, match="detect_qp: a lockstep solver takes no quadratic infeasibility tests"):
        ipm.IpmSolver(A, b, c, quad=g, detect_qp=True, lockstep=True)
    with pytest.raises(ValueError, match="detect_qp: the lockstep batch takes no quadratic infeasibility tests"):
        batches.solve_lockstep([], detect_qp=True)
    with pytest.raises(ValueError, match="detect_qp: the lockstep batch takes no quadratic infeasibility tests"):
        batch.solve_shard_lockstep([], [], detect_qp=True)
    # the refusals that remain with the flag set
    with pytest.raises(ValueError, match="correctors=2 takes no quadratic term"):
        ipm.IpmSolver(A, b, c, quad=g, detect_qp=True, correctors=2)
    with pytest.raises(ValueError, match='start="mehrotra" takes no free columns'):
        ipm.solve_with_info(A, b, c, quad=g, free=[0], detect_qp=True, start="mehrotra")
    # ... and, without it, the old ones word for word
    with pytest.raises(ValueError, match="quad: detect_infeasibility=True takes no quadratic term \\(the infeasibility tests are the LP's\\)"):
        ipm.IpmSolver(A, b, c, quad=g, detect_infeasibility=True)
    with pytest.raises(ValueError, match="quad: detect_infeasibility=True takes no quadratic term \\(the infeasibility tests are the LP's\\)"):
        ipm.solve_with_info(A, b, c, quad=g, free=[0], detect_infeasibility=True)
    with pytest.raises(ValueError, match="free: detect_infeasibility=True takes no free columns \\(the infeasibility tests are the LP's\\)"):
        handle.refuse_free([0], "detect_infeasibility=True", "the infeasibility tests are the LP's")
    with pytest.raises(ValueError, match="solve_factor_qp builds it"):
        ipm.solve_factor_qp(A, b, c, np.ones((3, 1)), quad=g, detect_qp=True)


def test_factor_qp_solution_maps_a_certificate():
    """factor_qp_solution on a hand-made record: kind 5 keeps y (m) and gets y_factor (k); kind 6 keeps x (n) and gets t (k)."""
    m, n, k = 2, 3, 2
    F, c_, g_ = np.ones((n, k)), np.ones(n + k), np.ones(n + k)
    xa, ya, sa = np.arange(5.0).reshape(-1, 1), np.arange(4.0).reshape(-1, 1), np.zeros((5, 1))
    cert = dict(kind="dual_infeasible", y=np.arange(4.0), z=np.arange(5.0), x=np.arange(5.0) + 10, normalization=2.0, violation=1e-9, k=7)
    info = dict(objective=1.0, certificate=cert)
    out = factor_qp.factor_qp_solution(xa, ya, sa, info, F, c_, g_, m, n)[3]["certificate"]
    assert out["x"].tolist() == [10, 11, 12] and out["t"].tolist() == [13, 14] and out["y"].tolist() == [0, 1] and out["y_factor"].tolist() == [2, 3]
    assert out["z"].tolist() == [0, 1, 2] and (out["kind"], out["normalization"], out["violation"], out["k"]) == ("dual_infeasible", 2.0, 1e-9, 7)
    assert len(cert["x"]) == 5                             # the input record is not changed
    assert "certificate" not in factor_qp.factor_qp_solution(xa, ya, sa, dict(objective=1.0), F, c_, g_, m, n)[3]
    assert factor_qp.factor_qp_solution(xa, ya, sa, dict(objective=1.0, certificate=None), F, c_, g_, m, n)[3]["certificate"] is None


def test_check_detect_qp():
    assert handle.check_detect_qp(False, None) is False and handle.check_detect_qp(True, np.ones(2)) is True
    assert handle.check_detect_qp(0, np.ones(2)) is False
    handle.refuse_detect_qp(False, "x", "y")
