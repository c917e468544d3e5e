"""Infeasibility detection on the device (IPM_FLAG_DETECT_INFEASIBILITY).

Every instance of tests/infeas_cases.py on every path it is meant to hit (fused small LP, dense, fused dense launch, sparse
envelope, sparse factor, bounded, lockstep batch): status 5 / 6 of the right kind within 100 iterations, a certificate that
verify_certificate confirms from the data to 1e-7, k of the detection = the iteration count.  The tests only read: a flagged
solve follows the unflagged one bit for bit until it stops, and no valid Netlib LP is ever classified infeasible."""
import os

import numpy as np
import pytest
from scipy import sparse

import infeas_cases as IC
from interiorpointmethod_amd import general_form as G
from interiorpointmethod_amd import solver as S
from interiorpointmethod_amd.solver import IpmSolver, LockstepBatch, verify_certificate

pytestmark = pytest.mark.gpu

TOL_CERT = 1e-7
MAX_K = 100


def _run(P, detect=True, max_iter=200, history=False, **kw):
    with IpmSolver(P["A"], P["b"], P["c"], ub=P["ub"], detect_infeasibility=detect, **kw) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=1e-8, max_iter=max_iter)
        out = dict(stats=st, cert=sv.certificate(), schedule=sv.schedule(), factor=sv.factor, state=sv.get_state())
        if history:
            out["history"] = sv.history()
        return out


def _check(P, r, name):
    st, cert = r["stats"], r["cert"]
    assert st["status"] == IC.KIND[P["kind"]], (name, S.STATUS_NAMES.get(st["status"]), st["iterations"])
    assert st["iterations"] <= MAX_K, (name, st["iterations"])
    assert cert is not None and cert["kind"] == P["kind"], name
    assert cert["k"] == st["iterations"], (name, cert["k"], st["iterations"])
    assert cert["normalization"] > 0 and cert["violation"] <= 1e-8, (name, cert)
    v = verify_certificate(P["A"], P["b"], P["c"], cert, ub=P["ub"])
    assert v <= TOL_CERT, (name, v, cert["violation"])


def _sparse(P):
    return dict(P, A=sparse.csc_matrix(P["A"]))


# ------------------------------------------------------------------------------------------- the fused small-LP kernel (m <= 128)
@pytest.mark.parametrize("name", ["primal_dense", "dual_dense", "afiro_dup_row", "afiro_neg_row", "afiro_ray_col",
                                  "bounded_primal", "bounded_dual"])
def test_fused_small_lp(name):
    P = _sparse(IC.small_instances()[name]())
    r = _run(P)
    assert r["schedule"]["fused_small"] == 1
    _check(P, r, name)


# ------------------------------------------------------------------------------------------- multi-kernel dense (plain and bounded)
@pytest.mark.parametrize("name", ["primal_dense", "dual_dense", "bounded_primal", "bounded_dual"])
def test_dense_multi_kernel(name):
    P = IC.small_instances()[name]()
    r = _run(P, dense=True)
    assert r["schedule"]["fused_small"] == 0
    _check(P, r, name)


def test_fused_dense_launch():
    """21 blocks of 128 rows: the stop test runs on the residual stream while the fused formation + factorization is in flight."""
    P = IC.large_dense()
    r = _run(P, dense=True, history=True)
    assert r["schedule"]["fused_factor"] == 1 and r["schedule"]["blocks"] == 21
    _check(P, r, "large_dense")
    # detection only reads: the unflagged solve stopped at the same iteration holds the same records and the same iterate
    k = r["stats"]["iterations"]
    r0 = _run(P, detect=False, max_iter=k, history=True)
    assert r0["stats"]["status"] == 2 and r0["stats"]["iterations"] == k
    assert r0["history"] == r["history"]
    for a, b in zip(r0["state"], r["state"]):
        assert np.array_equal(a, b)


def test_history_bitwise_on_the_dense_path():
    P = IC.dual_infeasible_dense()
    r = _run(P, dense=True, history=True)
    _check(P, r, "dual_dense")
    k = r["stats"]["iterations"]
    r0 = _run(P, detect=False, max_iter=k, history=True)
    assert r0["stats"]["iterations"] == k and r0["history"] == r["history"]
    for a, b in zip(r0["state"], r["state"]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------- mid-size sparse (m > 128)
@pytest.mark.parametrize("name", sorted(IC.mid_instances()))
@pytest.mark.parametrize("factor", ["dense", "sparse"])
def test_mid_sparse(name, factor):
    P = IC.mid_instances()[name]()
    r = _run(P, factor=factor)
    assert r["schedule"]["fused_small"] == 0 and r["factor"] == factor
    if factor == "dense":
        assert r["schedule"]["envelope"] in (0, 1)
    _check(P, r, name + "/" + factor)


def test_interior_sparse_and_general_form_verdicts():
    P = IC.afiro_negative_sum_row()
    assert S.interior_sparse(P["A"], P["b"], P["c"], detect_infeasibility=True) == np.inf
    Q = IC.afiro_free_ray_column()
    assert S.interior_sparse(Q["A"], Q["b"], Q["c"], detect_infeasibility=True) == -np.inf
    D = IC.dual_infeasible_dense()
    assert S.interior(D["A"], D["b"], D["c"], detect_infeasibility=True) == -np.inf
    # general form: x1 + x2 <= 1 and x1 + x2 = 3 (infeasible); y in get_Abc order (inequality row, then equality row)
    c = np.array([1.0, 1.0])
    kw = dict(Aeq=np.array([[1.0, 1.0]]), beq=np.array([3.0]), Aineq=np.array([[1.0, 1.0]]), bineq=np.array([1.0]))
    obj, info = G.new_interior_sparse(c, **kw, tol=1e-8, detect_infeasibility=True, return_info=True)
    assert obj == np.inf and info["status"] == 5
    A, b, cs, _ = G.standard_form(c, **kw)
    assert verify_certificate(A, b, cs, info["certificate"]) <= TOL_CERT
    # unbounded in general form, native bounds: min -x1 s.t. x1 - x2 = 0, x2 <= inf, x3 in [0, 1] (the ray avoids the bound)
    obj, info = G.new_interior_sparse(np.array([-1.0, 0.0, 0.0]), Aeq=np.array([[1.0, -1.0, 1.0]]), beq=np.array([0.5]),
                                      ub=np.array([np.inf, np.inf, 1.0]), tol=1e-8, bounds="native", detect_infeasibility=True,
                                      return_info=True)
    assert obj == -np.inf and info["status"] == 6
    xo = info["certificate"]["x_original"]
    assert xo[0] > 0 and abs(xo[0] - xo[1]) <= 1e-7 * xo[0] and xo[2] <= 1e-7


# ------------------------------------------------------------------------------------------- lockstep batch
def _solve_alone(P, detect):
    with IpmSolver(P["A"], P["b"], P["c"], lockstep=True, concurrent=True, factor="dense", detect_infeasibility=detect) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=1e-8, max_iter=200)
        return st, sv.certificate(), sv.get_state()


def test_lockstep_batch_mixed_with_unflagged():
    """Flagged mid-size instances and unflagged valid Netlib LPs in ONE batch: every LP gets the status, k, certificate and
    iterate that the same lockstep handle gets solved alone, bit for bit."""
    probs = [(nm, IC.mid_instances()[nm](), True) for nm in sorted(IC.mid_instances())]
    for nm in IC.MID_NETLIB:
        A, b, c = IC.netlib(nm)
        probs.append((nm, dict(A=A, b=b, c=c, ub=None, kind=None), False))
    svs = []
    try:
        for nm, P, det in probs:
            sv = IpmSolver(P["A"], P["b"], P["c"], lockstep=True, concurrent=True, factor="dense", detect_infeasibility=det)
            assert S.lockstep_eligible(sv), nm
            sv.init_state(1.0)
            svs.append(sv)
        with LockstepBatch(tol=1e-8, max_iter=200) as B:
            for sv in svs:
                B.add(sv)
            while B.active:
                B.step()
        got = [(sv.stats, sv.certificate(), sv.get_state()) for sv in svs]
    finally:
        for sv in svs:
            sv.close()
    for (nm, P, det), (st, cert, state) in zip(probs, got):
        st1, cert1, state1 = _solve_alone(P, det)
        assert st["status"] == st1["status"] and st["iterations"] == st1["iterations"], nm
        for a, b in zip(state, state1):
            assert np.array_equal(a, b), nm
        if det:
            _check(P, dict(stats=st, cert=cert), nm + "/lockstep")
            for key in ("y", "z", "x"):
                assert np.array_equal(cert[key], cert1[key]), (nm, key)
            assert (cert["normalization"], cert["violation"], cert["k"]) == (cert1["normalization"], cert1["violation"], cert1["k"])
        else:
            assert st["status"] not in (5, 6) and cert is None, nm


# ------------------------------------------------------------------------------------------- no false positives
HIGHS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netlib_highs_status.json")


def _same(u, v):
    return np.array_equal(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), equal_nan=True)


def _same_history(h1, h0):
    return len(h1) == len(h0) and all(r1.keys() == r0.keys() and all(_same(r1[k], r0[k]) for k in r1) for r1, r0 in zip(h1, h0))


def test_no_false_positive_on_netlib():
    """Every valid standard-form Netlib fixture, with detection and without.  Several of them are infeasible AS STANDARD-FORM
    fixtures (bounds of the general form dropped: BOEING1, FINNIS, ...; HiGHS verdicts in tests/golden/netlib_highs_status.json).
    An LP HiGHS solves is never classified; an infeasible one may only be classified primal infeasible, with a certificate that
    verifies.  Where nothing fires, status, k, objective and (x, y, s) are bitwise equal; where it fires at k, the history of the
    flagged solve is the first k records of the unflagged one, bit for bit."""
    import json
    verdict = json.load(open(HIGHS))
    bad, fired = [], []
    for nm in sorted(verdict):
        A, b, c = IC.netlib(nm)
        x1, y1, s1, i1 = S.solve_with_info(A, b, c, tol=1e-8, max_iter=300, detect_infeasibility=True, history=True)
        x0, y0, s0, i0 = S.solve_with_info(A, b, c, tol=1e-8, max_iter=300, history=True)
        if i1["status"] in (5, 6):
            fired.append(nm)
            cert = i1["certificate"]
            if verdict[nm] != 2 or i1["status"] != 5 or verify_certificate(A, b, c, cert) > TOL_CERT or cert["k"] != i1["iterations"]:
                bad.append((nm, "classified", verdict[nm], i1["status"]))
            k = i1["iterations"]
            if not (i0["iterations"] >= k and _same_history(i1["history"], i0["history"][:k])):
                bad.append((nm, "history differs before the detection"))
            continue
        if i1["certificate"] is not None:
            bad.append((nm, "certificate without a detection"))
        if (i1["status"], i1["iterations"]) != (i0["status"], i0["iterations"]) or not _same(i1["objective"], i0["objective"]) or \
                not (_same(x1, x0) and _same(y1, y0) and _same(s1, s0)):
            bad.append((nm, "differs", i0["status"], i0["iterations"], i1["status"], i1["iterations"]))
    print("detected (HiGHS: infeasible as standard form):", fired)
    assert not bad, bad


GEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "general")


def _load_general(name):
    z = np.load(os.path.join(GEN, name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


# the bounded general-form files the native path solves (tests/test_gpu_bounds.py)
NATIVE_OK = ["80BAU3B", "BOEING1", "BOEING2", "BORE3D", "CZPROB", "ETAMACRO", "FIT1P", "FORPLAN", "GANGES", "GFRD-PNC", "GROW15",
             "GROW22", "GROW7", "KB2", "MAROS", "NESM", "PILOT87", "PILOTNOV", "SEBA", "SHELL", "SIERRA", "STANDATA", "STANDMPS"]


def test_no_false_positive_on_bounded_general_form():
    bad = []
    for nm in NATIVE_OK:
        args = _load_general(nm)
        if not np.isfinite(np.ravel(args["ub"])).any():
            continue
        o1, i1 = G.new_interior_sparse(**args, tol=1e-8, bounds="native", start="mehrotra", return_info=True, detect_infeasibility=True)
        o0, i0 = G.new_interior_sparse(**args, tol=1e-8, bounds="native", start="mehrotra", return_info=True)
        if i1["status"] in (5, 6) or i1["certificate"] is not None:
            bad.append((nm, "classified", i1["status"]))
        if (i1["status"], i1["iterations"]) != (i0["status"], i0["iterations"]) or not _same(o1, o0) or not _same(i1["x"], i0["x"]):
            bad.append((nm, "differs", i0["status"], i0["iterations"], i1["status"], i1["iterations"]))
    assert not bad, bad


def test_certificate_state_errors():
    P = IC.afiro_free_ray_column()
    with IpmSolver(P["A"], P["b"], P["c"], detect_infeasibility=False) as sv:
        sv.init_state(1.0)
        sv.solve(tol=1e-8, max_iter=30)
        assert sv.stats["status"] in (2, 3) and sv.certificate() is None
        y, z, x, info = np.empty(sv.m), np.empty(sv.n), np.empty(sv.n), np.empty(4)
        code = sv._lib.ipm_get_certificate(sv._h, S._dptr(y), S._dptr(z), S._dptr(x), S._dptr(info))
        assert code == -5                                    # IPM_ERR_STATE
