"""Infeasibility detection for quadratic problems on the device (IPM_FLAG_DETECT_QUADRATIC, detect_qp=True).

The cases are tests/qp_infeas_cases.py (tests/test_qp_detect_host.py holds them, their certificates and the float64 host loop on
the CPU).  Here:

  1. whole solves on every case on the multi-kernel path -- dense 40 x 90 (36 x 86 augmented), CSC of about 130 x 300 on the
     envelope factor and with the sparse factor, one dense case of 21 blocks (fused launch, residual stream): the status is the host
     loop's kind, the iteration of the detection within 2 of the host loop's (the project's margin for iteration counts), cert["k"] ==
     iterations, cert["violation"] <= eps, verify_certificate <= TOL_CERT = 1e-7 (test_gpu_infeasibility.py's).  Negative cases:
     status 1 and (x, y, s, w, z) and history bit-identical to an unflagged quadratic handle.
  2. ONE stop test against the longdouble oracle where the loops change shape (qp_infeas_cases.EDGE): normalization and violation
     of the record against np.longdouble at the state read back, to the DETECT_TOL = 1e-12 of test_gpu_iteration_edges.py, with
     max g|x| (free column with x < 0, or barrier column) and the free columns' max |A^T y| (either sign) attained at column 0, 255,
     256, n - 1 of 40 x 600, in the second grid-stride trip of 8 x 16500, with bounded columns interleaved, at m = 1.  At the stop
     test of iteration 0 for every cell (a constructed state), and at iteration 1, 2 or 3 with eps between the oracle's ratios of
     consecutive iterates: the curvature cells from their own states (qp_infeas_cases.delayed); the free-column cells from an iterate
     of the host loop on a primal infeasible problem with free columns, the attaining column swapped to its place and given its sign
     (qp_infeas_cases.primal_delayed -- from the constructed states the primal ratio rises, so no eps separates a later iterate
     from the first).  K = 1, 2 and 3 at every one of the four columns of 40 x 600, both signs; the bounded and the second-trip
     cells at one K each.  m = 1 is held at iteration 0 (and the curvature cell at iteration 1): a 1 x 2 problem with a free column
     whose A^T y must vanish has a zero column there, and its curvature ratio falls too slowly for K = 2, 3.
  3. the one-workgroup path (quad_small / free_small): the same cells and whole solves at 1 and 8 tiles and n = 511, 513; solo
     against batch bit for bit; all twelve variants in one batch; a 64-member sweep with three infeasible members.
  4. invariants: repeats, check_every, what device memory held, scale="ruiz" against the host-prescaled problem, refine=2, both
     orders of the setters, the refusals that remain.
  5. solve_factor_qp(..., detect_qp=True): the mapped certificate against the ORIGINAL (A, b, c, F, g, ub), both kinds.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib
from interiorpointmethod_amd.solver import IpmSolver, verify_certificate

import equilibrate_oracle as EO
import free_qp_oracle as FO
import qp_infeas_cases as QC
from test_gpu_iteration_edges import DETECT_TOL, ULP2, _assert_all, _srel

pytestmark = pytest.mark.gpu

TOL_CERT = 1e-7
MARGIN_K = 2
STATUS = {"primal_infeasible": 5, "dual_infeasible": 6}


def _open(P, as_sparse=False, detect=True, **kw):
    A = sparse.csc_matrix(P["A"]) if as_sparse else P["A"]
    if detect:
        kw = dict(kw, detect_qp=True)
    return IpmSolver(A, P["b"], P["c"], ub=P["ub"], quad=P["g"], free=P["free"], **kw)


def _bits(sv):
    return [np.asarray(v).tobytes() for v in sv.get_state() + (sv.get_bound_state() or ())]


def _run(P, max_iter=200, **kw):
    with _open(P, **kw) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=1e-8, max_iter=max_iter)
        return dict(stats=st, cert=sv.certificate(), schedule=sv.schedule(), factor=sv.factor, bits=_bits(sv), history=sv.history(),
                    state=sv.get_state(), quadratic=sv.quadratic_nonzeros())


def _check_positive(name, P, r):
    st, cert = r["stats"], r["cert"]
    _, kind, k_host = QC.CASES[name]
    print("DETECT %s status %d k %d (host %d) violation %.3e" % (name, st["status"], st["iterations"], k_host, cert["violation"] if cert else np.nan))
    assert st["status"] == STATUS[kind], (name, st["status"], st["iterations"])
    assert abs(st["iterations"] - k_host) <= MARGIN_K, (name, st["iterations"], k_host)
    assert cert is not None and cert["kind"] == kind and cert["k"] == st["iterations"]
    assert cert["normalization"] > 0 and cert["violation"] <= QC.EPS, (name, cert["violation"])
    v = verify_certificate(P["A"], P["b"], P["c"], cert, ub=P["ub"], g=P["g"], free=P["free"])
    assert v <= TOL_CERT, (name, v)


def _check_negative(name, P, r, **kw):
    """Status 1, and the bits of the same solve on an unflagged quadratic handle."""
    assert r["stats"]["status"] == 1 and r["cert"] is None, (name, r["stats"]["status"])
    assert abs(r["stats"]["iterations"] - QC.CASES[name][2]) <= MARGIN_K
    r0 = _run(P, detect=False, **kw)
    assert r0["stats"]["status"] == 1 and r0["stats"]["iterations"] == r["stats"]["iterations"]
    assert r0["bits"] == r["bits"] and r0["history"] == r["history"], name


# ---- 1. whole solves, multi-kernel path ----------------------------------------------------------------------------------------
DENSE_NAMES = [nm for nm in QC.SMALL if not nm.startswith(("sparse", "tile"))]


@pytest.mark.parametrize("name", DENSE_NAMES)
def test_whole_solve_dense(name):
    P = QC.get(name)
    r = _run(P, dense=True)
    assert r["schedule"]["fused_small"] == 0 and r["quadratic"] > 0
    if QC.CASES[name][1] is None:
        _check_negative(name, P, r, dense=True)
    else:
        _check_positive(name, P, r)


@pytest.mark.parametrize("factor", ["dense", "sparse"])
@pytest.mark.parametrize("name", ["sparse-primal", "sparse-dual"])
def test_whole_solve_sparse(name, factor):
    P = QC.get(name)
    r = _run(P, as_sparse=True, factor=factor)
    assert r["schedule"]["fused_small"] == 0 and r["factor"] == factor
    _check_positive(name, P, r)


def test_whole_solve_fused_launch_and_residual_stream():
    """21 blocks: the stop test runs on the residual stream while the fused formation + factorization is in flight (the done_f latch).
    Detection only reads: the unflagged quadratic solve stopped at the same iteration holds the same records and the same iterate."""
    P = QC.get("large-dense")
    r = _run(P, dense=True)
    assert r["schedule"]["fused_factor"] == 1 and r["schedule"]["blocks"] == 21
    _check_positive("large-dense", P, r)
    k = r["stats"]["iterations"]
    r0 = _run(P, detect=False, dense=True, max_iter=k)
    assert r0["stats"]["status"] == 2 and r0["stats"]["iterations"] == k
    assert r0["history"] == r["history"] and r0["bits"] == r["bits"]


# ---- 2. one stop test against the longdouble oracle ----------------------------------------------------------------------------
def _edge_solver(case, g, free, small, tol, **kw):
    as_sparse = small or case.n > 16384
    A = sparse.csc_matrix(case.A) if as_sparse else case.A
    if small:
        kw = dict(kw, free_small=True)
    sv = IpmSolver(A, case.b, case.c, ub=case.ub(), quad=g, free=free, detect_qp=True, infeasibility_tol=tol, **kw)
    try:
        assert sv.schedule()["fused_small"] == (1 if small else 0)
    except Exception:
        sv.close()
        raise
    return sv


def _check_record(cell, sv, at, g, free, kind, st, k):
    """The record of a detection at the stop test of iteration k against the oracle's quantities of the iterate `at` (the device state
    of that moment), and the certificate's vectors against that state."""
    q = QC.quantities(at, g, free)
    primal = kind == "primal"
    cert = sv.certificate()
    assert st["status"] == (5 if primal else 6) and st["iterations"] == k, (cell, st["status"], st["iterations"])
    assert cert is not None and cert["k"] == k and cert["kind"] == ("primal_infeasible" if primal else "dual_infeasible")
    nrm, viol = (q["beta"], q["vp"] / q["beta"]) if primal else (q["gamma"], q["vd"] / q["gamma"])
    _assert_all(cell, {"normalization": _srel(cert["normalization"], nrm), "violation": _srel(cert["violation"], viol)},
                {"normalization": DETECT_TOL, "violation": DETECT_TOL})
    d = cert["normalization"]
    if primal:
        assert np.all(np.abs(cert["y"] - at.y / d) <= ULP2 * np.abs(at.y / d)) and np.all(cert["x"] == 0)
        assert np.all(np.abs(cert["z"] - at.z / d) <= ULP2 * np.abs(at.z / d))
    else:
        assert np.all(np.abs(cert["x"] - at.x / d) <= ULP2 * np.abs(at.x / d))
        assert np.all(cert["y"] == 0) and np.all(cert["z"] == 0)


def _state_of(sv, case):
    x, y, s = (v.ravel().copy() for v in sv.get_state())
    w, z = (v.ravel().copy() for v in sv.get_bound_state()) if case.bounded else (case.w, case.z)
    return case.copy(x=x, y=y, s=s, w=w, z=z)


def _small_ok(name):
    return "16500" not in name          # (8 x 16500 has a product list of its own size class; the small path's cells are the others)


EDGE_CELLS = [(nm, False) for nm in QC.EDGE] + [(nm, True) for nm in QC.EDGE if _small_ok(nm)]


@pytest.mark.parametrize("name,small", EDGE_CELLS, ids=["%s/%s" % (nm, "small" if sm else "multi") for nm, sm in EDGE_CELLS])
def test_stop_test_against_the_oracle(name, small):
    """prepare_*_detect_kernel + stop_test_*_detect_kernel (small: residual_cols and stop_test of small_lp_body<.., true, true, ..>) at
    a known iterate.  The stop test skips detection under `force`, so the state is set and solve() called, not iterate()."""
    case, g, free = QC.edge(name)
    kind = QC.EDGE[name][1]
    with _edge_solver(case, g, free, small, (0.5, 0.5)) as sv:
        sv.set_state(*case.state())
        st = sv.solve(tol=1e-8, max_iter=5)
        at = _state_of(sv, case)
        fm = FO.free_mask(free, case.n)
        assert np.array_equal(at.x, case.x) and np.array_equal(at.y, case.y) and np.array_equal(at.s, np.where(fm, 0.0, case.s))      # the iterate has not moved
        _check_record(name, sv, case, g, free, kind, st, 0)


# (1 x 2 offers K = 1 only: from there on its ratio falls by less than the margin)
DELAYED_CELLS = [(nm, K, sm) for nm in QC.EDGE if nm.startswith("curv/") and "barrier" not in nm for K in (1, 2, 3)
                 for sm in ((False, True) if _small_ok(nm) else (False,)) if (K == 1 or "1x2" not in nm)]


@pytest.mark.parametrize("name,K,small", DELAYED_CELLS, ids=["%s/K%d/%s" % (nm, K, "small" if sm else "multi") for nm, K, sm in DELAYED_CELLS])
def test_stop_test_fires_at_iteration_k(name, K, small):
    """The dual test fires first at the stop test of iteration K: the partials (small: the running sums and maxima) of the tests after
    K iterations, against the oracle at the state read back.  The iterate at detection is iterate(K)'s of the same handle, bit for bit."""
    d = QC.delayed(name, K)
    assert d is not None and d["kind"] == "dual"
    case, g, free = d["case"], d["g"], d["free"]
    with _edge_solver(case, g, free, small, d["tol"]) as sv:
        sv.set_state(*case.state())
        st = sv.solve(tol=1e-8, max_iter=5)
        at = _state_of(sv, case)
        print("DELAYED %s K %d tol %s ratios %s at detection %s" % (name, K, d["tol"], d["ratios"], QC.ratios(at, g, free)))
        _check_record("%s/K%d" % (name, K), sv, at, g, free, "dual", st, K)
        assert len(sv.history()) == K
        fired = _bits(sv)
        sv.set_state(*case.state())
        sv.iterate(K)
        assert _bits(sv) == fired, name


PRIMAL_DELAYED_CELLS = [(nm, sm) for nm in QC.PRIMAL_DELAYED for sm in ((False, True) if _small_ok(nm) else (False,))]


@pytest.mark.parametrize("name,small", PRIMAL_DELAYED_CELLS, ids=["%s/%s" % (nm, "small" if sm else "multi") for nm, sm in PRIMAL_DELAYED_CELLS])
def test_primal_stop_test_fires_at_iteration_k(name, small):
    """The primal test fires first at the stop test of iteration K with max |A^T y| over the free columns attained at the cell's
    column, with the cell's sign: against the oracle at the state read back, and bit for bit the iterate of iterate(K).
    The start is an EARLY iterate of the host loop (qp_infeas_cases.primal_delayed): |y| is still O(10) there and (A^T y)_j of the free
    column a well-conditioned sum (kappa = sum |a_ij y_i| / |(A^T y)_j| <= 62 over the cells, so (m + 2) 2^-53 kappa <= 3e-13), and the
    bound is DETECT_TOL, unchanged."""
    d = QC.primal_delayed(name)
    case, g, free, K = d["case"], d["g"], d["free"], d["K"]
    with _edge_solver(case, g, free, small, d["tol"]) as sv:
        sv.set_state(*case.state())
        st = sv.solve(tol=1e-8, max_iter=6)
        at = _state_of(sv, case)
        q = QC.quantities(at, g, free)
        print("DELAYED %s tol %s ratios %s at detection %s column %s" % (name, d["tol"], d["ratios"], QC.ratios(at, g, free), q["col_free"]))
        assert q["col_free"] == QC.PRIMAL_DELAYED[name][4] and np.sign(float(q["aty_free"])) == QC.PRIMAL_DELAYED[name][5] and q["vp"] == q["free_max"]
        assert d["kappa"] <= 100
        _check_record(name, sv, at, g, free, "primal", st, K)
        assert len(sv.history()) == K
        fired = _bits(sv)
        sv.set_state(*case.state())
        sv.iterate(K)
        assert _bits(sv) == fired, name


# ---- 3. the one-workgroup path -------------------------------------------------------------------------------------------------
SMALL_NAMES = [nm for nm in QC.SMALL if not nm.startswith("sparse")]


def _small_kw(P):
    return dict(free_small=True) if P["free"] is not None else dict(quad_small=True)


def _collect(sv):
    return _bits(sv), sv.history(), {k: v for k, v in sv.stats.items() if k != "solve_ms"}, sv.certificate()


def _same_cert(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(np.array_equal(a[k], b[k]) for k in ("x", "y", "z")) and all(a[k] == b[k] for k in ("kind", "normalization", "violation", "k"))


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_small_path_whole_solve(name):
    P = QC.get(name)
    kw = _small_kw(P)
    r = _run(P, as_sparse=True, **kw)
    assert r["schedule"]["fused_small"] == 1, name
    if QC.CASES[name][1] is None:
        _check_negative(name, P, r, as_sparse=True, **kw)
    else:
        _check_positive(name, P, r)


def _variant_members():
    """One member per kernel variant of the small path (bounded x detect / term / free columns): name -> (P, options)."""
    import infeas_cases as IC
    lp, lpb = IC.dual_infeasible_dense(), IC.bounded_dual_infeasible()
    none = lambda P: dict(P, g=None, free=None)          # noqa: E731
    mem = {
        "lp": (none(lp), {}), "lp-bounded": (none(lpb), {}),
        "lp-detect": (none(lp), dict(detect_infeasibility=True)), "lp-bounded-detect": (none(lpb), dict(detect_infeasibility=True)),
        "qp": (QC.get("sep-dual/0"), dict(quad_small=True)), "qp-bounded": (QC.get("sep-dual-bounded/0"), dict(quad_small=True)),
        "free": (QC.get("factor-primal/0"), dict(free_small=True)), "free-bounded": (QC.get("factor-dual/0"), dict(free_small=True)),
        "qp-detect": (QC.get("sep-dual/1"), dict(quad_small=True, detect_qp=True)),
        "qp-bounded-detect": (QC.get("sep-bounded-primal"), dict(quad_small=True, detect_qp=True)),
        "free-detect": (QC.get("factor-primal/1"), dict(free_small=True, detect_qp=True)),
        "free-bounded-detect": (QC.get("factor-dual/1"), dict(free_small=True, detect_qp=True)),
    }
    return mem


def _member(P, opts):
    return IpmSolver(sparse.csc_matrix(P["A"]), P["b"], P["c"], ub=P["ub"], quad=P["g"], free=P["free"], **opts)


def test_batch_of_all_twelve_variants_is_bitwise_the_solo_solves():
    """Flagged QPs, unflagged QPs, LPs and detecting LPs in ONE ipm_solve_small_batch call: each member is its own ipm_solve, bit for
    bit -- state, history, statistics and certificate.  (The unflagged members run to the cap of 30 iterations or to nan.)"""
    mem = _variant_members()
    solo = {}
    for nm, (P, opts) in mem.items():
        with _member(P, opts) as sv:
            assert sv.schedule()["fused_small"] == 1, nm
            sv.init_state(1.0)
            sv.solve(tol=1e-8, max_iter=30)
            solo[nm] = _collect(sv)
    svs = []
    try:
        for nm, (P, opts) in mem.items():
            svs.append(_member(P, opts))
            svs[-1].init_state(1.0)
        variants = {(bool(sv.bounded), sv.detect_infeasibility, sv.quadratic_nonzeros() > 0, sv._n_free > 0) for sv in svs}
        assert len(variants) == 12
        ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=30)
        for nm, sv in zip(mem, svs):
            bits, hist, stats, cert = _collect(sv)
            assert bits == solo[nm][0] and hist == solo[nm][1], nm
            assert stats == solo[nm][2] or all(stats[k] == solo[nm][2][k] or (stats[k] != stats[k] and solo[nm][2][k] != solo[nm][2][k]) for k in stats), nm
            assert _same_cert(cert, solo[nm][3]), nm
            if "detect" in nm:
                assert stats["status"] in (5, 6) and cert["k"] == stats["iterations"], (nm, stats["status"])
            else:
                assert stats["status"] in (2, 3) and cert is None, (nm, stats["status"])
    finally:
        for sv in svs:
            sv.close()


def test_tile_cases_solo_against_batch():
    """The 1-tile and 8-tile cases at n = 511 / 513 (and one 40 x 90 member between them) in ONE batch call: each is its own solve,
    bit for bit -- state, history, statistics, certificate."""
    names = QC.TILES + ["sep-bounded-primal"]
    solo = {}
    for nm in names:
        P = QC.get(nm)
        with _open(P, as_sparse=True, **_small_kw(P)) as sv:
            assert sv.schedule()["fused_small"] == 1, nm
            sv.init_state(1.0)
            sv.solve(tol=1e-8, max_iter=200)
            solo[nm] = _collect(sv)
    svs = []
    try:
        for nm in names:
            P = QC.get(nm)
            svs.append(_open(P, as_sparse=True, **_small_kw(P)))
            svs[-1].init_state(1.0)
        assert {(sv.m + 15) // 16 for sv in svs} >= {1, 8} and {sv.n for sv in svs} >= {511, 513}
        ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=200)
        for nm, sv in zip(names, svs):
            bits, hist, stats, cert = _collect(sv)
            assert bits == solo[nm][0] and hist == solo[nm][1] and stats == solo[nm][2] and _same_cert(cert, solo[nm][3]), nm
            assert stats["status"] == STATUS[QC.CASES[nm][1]] and cert["k"] == stats["iterations"], nm
    finally:
        for sv in svs:
            sv.close()


def test_sweep_with_three_infeasible_members():
    problems = QC.return_target_sweep()
    out = ipm.solve_small_factor_qp_batch_detect(problems, tol=1e-8, max_iter=200)
    ref = ipm.solve_small_factor_qp_batch(problems[:-3], tol=1e-8, max_iter=200)
    for i, (x, y, s, info) in enumerate(out[:-3]):
        x0, y0, s0, info0 = ref[i]
        assert info["status"] == 1 and info["certificate"] is None and info["quadratic_path"] == "one-workgroup", (i, info["status"])
        assert x.tobytes() == x0.tobytes() and y.tobytes() == y0.tobytes() and s.tobytes() == s0.tobytes() and info["iterations"] == info0["iterations"], i
    for (A, b, c, F, g), (x, y, s, info) in zip(problems[-3:], out[-3:]):
        cert = info["certificate"]
        assert info["status"] == 5 and cert["kind"] == "primal_infeasible" and cert["k"] == info["iterations"] <= 60, (info["status"], info["iterations"])
        assert cert["y"].shape == (2,) and cert["y_factor"].shape == (4,)
        assert verify_certificate(A, b, c, cert, g=g, F=F) <= TOL_CERT


# ---- 4. invariants -------------------------------------------------------------------------------------------------------------
INVARIANT_NAMES = ["sep-bounded-primal", "factor-dual/0"]


@pytest.mark.parametrize("name", INVARIANT_NAMES)
def test_repeat_check_every_and_stale_memory(name, monkeypatch):
    P = QC.get(name)
    base = _run(P, dense=True)
    _check_positive(name, P, base)
    key = lambda r: (r["bits"], r["history"], r["stats"]["status"], r["stats"]["iterations"], r["cert"]["normalization"], r["cert"]["violation"],          # noqa: E731
                     r["cert"]["x"].tobytes(), r["cert"]["y"].tobytes(), r["cert"]["z"].tobytes())
    assert key(_run(P, dense=True)) == key(base)
    assert key(_run(P, dense=True, check_every=1)) == key(base) and key(_run(P, dense=True, check_every=7)) == key(base)
    for fill in ("0", "255"):
        monkeypatch.setenv("IPM_TEST_ALLOC_FILL", fill)
        assert key(_run(P, dense=True)) == key(base), fill
    monkeypatch.delenv("IPM_TEST_ALLOC_FILL")
    with _open(P, dense=True) as sv:                       # a second solve of the same handle from a fresh state
        for _ in range(2):
            sv.init_state(1.0)
            sv.solve(tol=1e-8, max_iter=200)
            assert _bits(sv) == base["bits"] and sv.certificate()["violation"] == base["cert"]["violation"]


@pytest.mark.parametrize("name", INVARIANT_NAMES)
def test_refine_is_allowed(name):
    P = QC.get(name)
    r = _run(P, dense=True, refine=2)
    _check_positive(name, P, r)


@pytest.mark.parametrize("name", ["sep-bounded-primal", "factor-dual/0", "factor-primal/0"])
def test_ruiz_is_the_host_prescaled_problem(name):
    """scale="ruiz": the tests act on the SCALED problem (the record's normalization and violation are the scaled problem's, equal to
    the prescaled twin's bit for bit); the certificate's vectors leave in the caller's units and verify against the caller's data."""
    P = QC.get(name)
    rs = np.ldexp(1.0, np.random.default_rng(3).integers(-6, 7, P["A"].shape[0]))       # badly scaled rows: something to equilibrate
    A, b = P["A"] * rs[:, None], P["b"] * rs
    er, ec, changed = EO.ruiz(A, 16)
    assert changed > 0
    R, Cc = EO.factors(er, ec)
    A2, b2, c2, u2 = EO.prescale(A, b, P["c"], P["ub"], er, ec)
    g2 = P["g"] * Cc * Cc
    with IpmSolver(A, b, P["c"], ub=P["ub"], quad=P["g"], free=P["free"], detect_qp=True, dense=True, scale="ruiz") as s1, \
            IpmSolver(A2, b2, c2, ub=u2, quad=g2, free=P["free"], detect_qp=True, dense=True) as s2:
        for sv in (s1, s2):
            sv.init_state(1.0)
            sv.solve(tol=1e-8, max_iter=200)
        c1, c2_ = s1.certificate(), s2.certificate()
        assert s1.stats["status"] == s2.stats["status"] == STATUS[P["kind"]] and s1.stats["iterations"] == s2.stats["iterations"]
        assert s1.history() == s2.history()
        assert (c1["normalization"], c1["violation"], c1["k"]) == (c2_["normalization"], c2_["violation"], c2_["k"])
        assert np.array_equal(c1["x"], Cc * c2_["x"]) and np.array_equal(c1["y"], R * c2_["y"]) and np.array_equal(c1["z"], c2_["z"] / Cc)
        assert verify_certificate(A, b, P["c"], c1, ub=P["ub"], g=P["g"], free=P["free"]) <= TOL_CERT


def test_both_orders_of_the_setters():
    P = QC.get("factor-dual/0")
    base = _run(P, dense=True)
    recs = []
    for order in ("quad-first", "free-first"):
        with IpmSolver(P["A"], P["b"], P["c"], ub=P["ub"], quad=np.ones(len(P["c"])), detect_qp=True, dense=True) as sv:
            if order == "free-first":
                sv.set_quadratic(None)                      # cleared: the LP code; the set comes before its term
                sv.set_free(P["free"])
                sv.set_quadratic(P["g"])
            else:
                sv.set_quadratic(P["g"])
                sv.set_free(P["free"])
            sv.init_state(1.0)
            st = sv.solve(tol=1e-8, max_iter=200)
            recs.append((_bits(sv), sv.history(), st["status"], sv.certificate()["violation"]))
    assert recs[0] == recs[1] == (base["bits"], base["history"], 6, base["cert"]["violation"])


def test_refusals_that_remain():
    P = QC.get("factor-dual/0")
    lib = _lib.load()
    for flags, text in ((_lib.FLAG_DETECT_QUADRATIC, b"IPM_FLAG_DETECT_QUADRATIC without IPM_FLAG_DETECT_INFEASIBILITY"),
                        (_lib.FLAG_DETECT_QUADRATIC | _lib.FLAG_DETECT_INFEASIBILITY | _lib.FLAG_LOCKSTEP, b"IPM_FLAG_DETECT_QUADRATIC with IPM_FLAG_LOCKSTEP")):
        opts = _lib.Options()
        lib.ipm_default_options(C.byref(opts))
        opts.flags = flags
        h = C.c_void_p()
        code = lib.ipm_create(0, 4, 8, C.byref(opts), None, 0, None, C.byref(h))
        assert code == -1 and not h.value and text in lib.ipm_last_error(None), lib.ipm_last_error(None)
    with _open(P, dense=True) as sv:
        with pytest.raises(ipm.IpmError, match="quadratic term"):
            sv.set_correctors(2)
        with pytest.raises(ipm.IpmError, match="free columns"):
            sv.init_state_mehrotra()
    # without the new flag the setters refuse a detecting handle with the words they had
    with IpmSolver(P["A"], P["b"], P["c"], ub=P["ub"], detect_infeasibility=True, dense=True) as sv:
        with pytest.raises(ipm.IpmError, match="the dual ray of a QP also needs g o x = 0; the tests are not restated"):
            sv.set_quadratic(P["g"])
        with pytest.raises(ipm.IpmError, match="the tests are the LP's and are not restated"):
            sv.set_free(P["free"])


# ---- 5. solve_factor_qp --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["factor-primal/0", "factor-dual/0", "factor-curved/0"])
def test_solve_factor_qp_maps_the_certificate(name):
    P = QC.get(name)
    O, F = P["orig"], P["F"]
    m, n = O["A"].shape
    x, y, s, info = ipm.solve_factor_qp(O["A"], O["b"], O["c"], F, g=O["g"], ub=O["ub"], detect_qp=True, dense=True, max_iter=200)
    kind = QC.CASES[name][1]
    if kind is None:
        assert info["status"] == 1 and info["certificate"] is None
        return
    cert = info["certificate"]
    assert info["status"] == STATUS[kind] and cert["kind"] == kind and cert["k"] == info["iterations"]
    assert cert["y"].shape == (m,) and cert["y_factor"].shape == (6,) and cert["x"].shape == (n,) and cert["t"].shape == (6,) and cert["z"].shape == (n,)
    v = verify_certificate(O["A"], O["b"], O["c"], cert, ub=O["ub"], g=O["g"], F=F)
    print("FACTOR %s status %d k %d verify %.3e" % (name, info["status"], info["iterations"], v))
    assert v <= TOL_CERT
    if P["ub"] is None:                                    # (interior_sparse takes no bounds)
        assert ipm.interior_sparse(P["A"], P["b"], P["c"], quad=P["g"], free=P["free"], detect_qp=True) == np.inf


def test_interior_sparse_verdicts():
    """+inf for a QP detected infeasible, -inf for one detected unbounded, the objective for one that has an optimum."""
    P, D, N = QC.get("sep-primal/0"), QC.get("sep-dual/0"), QC.get("curved-everywhere")
    assert P["ub"] is None and D["ub"] is None and N["ub"] is None
    assert ipm.interior_sparse(P["A"], P["b"], P["c"], quad=P["g"], detect_qp=True) == np.inf
    assert ipm.interior_sparse(D["A"], D["b"], D["c"], quad=D["g"], detect_qp=True) == -np.inf
    v = ipm.interior_sparse(N["A"], N["b"], N["c"], tol=1e-8, quad=N["g"], detect_qp=True)      # (the drop-in's default tol is the reference's 1e-20)
    assert np.isfinite(v) and v == ipm.interior_sparse(N["A"], N["b"], N["c"], tol=1e-8, quad=N["g"])
