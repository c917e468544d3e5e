"""The separable convex QP on the device (ipm_set_quadratic): min c.x + 1/2 x.diag(g) x, A x = b, 0 <= x (<= u).

1. One iteration against the longdouble oracle of tests/qp_oracle.py, element by element, on the quantities and with the comparisons
   of tests/test_gpu_iteration_edges.py, at the shapes where the four Quad kernels (csrc/vector_ops.h) can go wrong: the first
   grid-stride trip with one column in the last block (129 x 16385 bounded), 400 x 520 bounded, 520 x 600 plain, 130 x 300 as CSC on
   the envelope factor and on the sparse factor, 60 x 150 as CSC (which must NOT take the one-workgroup small path).  g = 0 on every
   second column, so LP and QP columns mix in one wave.  Also: one step length, and the history's objective is the QP's.
2. Whole solves of workloads.separable_qp problems with a constructed optimum, against the float64 host loop of qp_oracle.
3. Invariants: bitwise repeat, clearing restores the LP bit for bit, independence from check_every, equilibration against the
   host-prescaled problem (g C^2), the getter.
4. The refusals the library decides, in both orders.

Bounds of part 1: test_gpu_iteration_edges._bound -- 100 x the maxima observed there, floor 1e-12 (under which
tests/test_qp_oracle_host.py holds the float64 restatement to the oracle on every case used here).
Bounds of part 2: iterations within 2 of the host loop's (the suite's allowance); the stop test's three inequalities recomputed in
longdouble hold with a factor 2 (the device passed them on that state; only summation order differs); ||x - x*|| / ||x*|| and the
objective within 100 x the host loop's own error on that problem, floor 1e-9.

Observed maxima on MI355X (first run of this file; every quantity stayed under its bound on that run, so no bound was replaced), per
quantity over the cells of part 1, and the cell that gave it (OBSERVED_QP below):
    dxa 5.4e-14, dsa 2.6e-14, dya 1.8e-14, dx 4.2e-14, ds 5.8e-14, dy 1.3e-14, A^T dy 3.4e-15, x 1.6e-14, s 2.9e-14      520 x 600
    A^T dya 3.0e-15, dw 3.0e-14, dz 4.4e-14, w 1.1e-14, z 2.1e-14, A^T y 2.3e-14, y 2.3e-14, alpha_aff_p/d 1.8e-15, alpha_p/d
    3.1e-14, sigma 3.3e-15                                                                                     400 x 520 bounded
    mu 1.9e-16, gap 1.4e-16, objective 1.4e-16, rp_norm 1.2e-16, rd_norm 1.8e-16                           129 x 16385 bounded
Whole solves (OBSERVED_SOLVES): the device's iteration counts equal the host loop's (12, 12, 12, 12, 13), and its errors against the
constructed optimum equal the host loop's to two digits: x 2.2e-12 / 4.5e-12 / 3.7e-12 (both sparse paths) / 5.7e-13.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, workloads

import equilibrate_oracle as EO
import iteration_oracle as IO
import qp_oracle as Q
from test_gpu_iteration_edges import _assert_all, _bound, _srel

pytestmark = pytest.mark.gpu

# the maxima of the first run of this file on an MI355X, for the record (the bounds are _bound's, not multiples of these)
OBSERVED_QP = {"dxa": 5.4e-14, "dsa": 2.6e-14, "ATdya": 3.0e-15, "dya": 1.8e-14, "dx": 4.2e-14, "ds": 5.8e-14, "dw": 3.0e-14, "dz": 4.4e-14,
               "ATdy": 3.4e-15, "dy": 1.3e-14, "x": 1.6e-14, "s": 2.9e-14, "w": 1.1e-14, "z": 2.1e-14, "ATy": 2.3e-14, "y": 2.3e-14,
               "alpha_aff_p": 1.8e-15, "alpha_aff_d": 1.8e-15, "alpha_p": 3.1e-14, "alpha_d": 3.1e-14, "mu": 1.9e-16, "sigma": 3.3e-15,
               "gap": 1.4e-16, "objective": 1.4e-16, "rp_norm": 1.2e-16, "rd_norm": 1.8e-16}
OBSERVED_SOLVES = {"300x700": (12, 2.2e-12), "300x700bm": (12, 4.5e-12), "200x520b": (12, 3.7e-12), "2560x5120": (13, 5.7e-13)}      # (iterations, x error)


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ---- 1. one iteration against the oracle ------------------------------------------------------------------------------------
def check_qp_iteration(cell, sv, case, g, o):
    AT = case.A.T
    e, bound = {}, {}

    def vec(k, got, want):
        e[k], bound[k] = IO.rel(got, want), _bound(k)

    def scal(k, got, want):
        e[k], bound[k] = _srel(got, want), _bound(k)

    assert np.array_equal(sv.quadratic(), g) and sv.quadratic_nonzeros() == int((g > 0).sum())
    sv.set_state(*case.state())
    dxa, dya, dsa = sv.newton_direction(False)
    st = dict(sv.stats)
    vec("dxa", dxa, o["dxa"]); vec("dsa", dsa, o["dsa"]); vec("ATdya", AT @ dya.ravel(), o["atdya"]); vec("dya", dya, o["dya"])
    scal("aff.alpha_aff_p", st["alpha_aff_p"], o["alpha_aff_p"]); scal("aff.alpha_aff_d", st["alpha_aff_d"], o["alpha_aff_d"])
    scal("aff.mu", st["mu"], o["mu"])
    assert st["alpha_aff_p"] == st["alpha_aff_d"]
    dx, dy, ds = sv.newton_direction(True)
    st = dict(sv.stats)
    vec("dx", dx, o["dx"]); vec("ds", ds, o["ds"]); vec("ATdy", AT @ dy.ravel(), o["atdy"]); vec("dy", dy, o["dy"])
    scal("cor.mu", st["mu"], o["mu"]); scal("cor.sigma", st["sigma"], o["sigma"])

    sv.set_state(*case.state())
    st = sv.iterate(1)
    x, y, s = sv.get_state()
    vec("x", x, o["xn"]); vec("s", s, o["sn"]); vec("ATy", AT @ y.ravel(), o["atyn"]); vec("y", y, o["yn"])
    scal("alpha_p", st["alpha_p"], o["alpha_p"]); scal("alpha_d", st["alpha_d"], o["alpha_d"])
    if case.bounded:
        w, z = sv.get_bound_state()
        vec("w", w, o["wn"]); vec("z", z, o["zn"])
        U = case.U
        assert np.all(w.ravel()[~U] == 0) and np.all(z.ravel()[~U] == 0)
        vec("dw", (w.ravel() - case.w) / st["alpha_p"], o["dw"]); vec("dz", (z.ravel() - case.z) / st["alpha_d"], o["dz"])
    else:
        assert sv.get_bound_state() is None
    hist = sv.history()
    assert len(hist) == 1 and hist[0]["k"] == 0 and st["iterations"] == 1
    h = hist[0]
    for k in ("gap", "mu", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "objective"):
        scal("hist." + k, h[k], o[k])                                      # (objective: the oracle's c.x + 1/2 x.G x)
    e["hist.rp_norm"], bound["hist.rp_norm"] = IO.residual_rel(h["rp_norm"], o["rp_norm"], o["b_norm"]), _bound("rp_norm")
    e["hist.rd_norm"], bound["hist.rd_norm"] = IO.residual_rel(h["rd_norm"], o["rd_norm"], o["c_norm"]), _bound("rd_norm")
    assert h["alpha_p"] == st["alpha_p"] and h["alpha_d"] == st["alpha_d"]
    assert st["alpha_p"] == st["alpha_d"] and h["alpha_aff_p"] == h["alpha_aff_d"]                 # ONE step length, exactly
    # the term is really in the objective: the LP's c.x differs from it by far more than the bound
    assert abs(float(np.asarray(case.c, dtype=IO.LD) @ np.asarray(case.x, dtype=IO.LD)) - h["objective"]) > 1e-3 * abs(h["objective"])
    _assert_all(cell, e, bound)


CELLS = [("dense/129x16385b", False, None), ("dense/400x520b", False, None), ("dense/520x600", False, None),
         ("sparse/130x300b", True, "dense"), ("sparse/130x300b", True, "sparse"), ("sparse/60x150", True, None)]


@pytest.mark.parametrize("name,as_sparse,factor", CELLS, ids=["%s%s" % (c[0], "-" + c[2] if c[2] else "") for c in CELLS])
def test_one_iteration(name, as_sparse, factor):
    case, g = Q.get(name)
    A = sparse.csc_matrix(case.A) if as_sparse else case.A
    kw = {} if factor is None else {"factor": factor}
    with ipm.IpmSolver(A, case.b, case.c, ub=case.ub(), quad=g, **kw) as sv:
        sch = sv.schedule()
        assert sch["fused_small"] == 0 and sv.sparse == as_sparse and sv.bounded == int(case.U.sum())
        if factor == "sparse":
            assert sv.factor == "sparse" and sv.factor_info()["panels"] >= 1
        elif as_sparse:
            assert sv.factor == "dense" and sch["blocks"] == (case.m + 127) // 128
        check_qp_iteration("%s/factor=%s" % (name, factor), sv, case, g, Q.oracle(name))


# ---- 2. whole solves --------------------------------------------------------------------------------------------------------
def _solve(name, as_sparse=False, **kw):
    A, b, c, g, u, xs, ys = Q.problem(name)
    with ipm.IpmSolver(sparse.csc_matrix(A) if as_sparse else A, b, c, ub=u, quad=g, **kw) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=Q.TOL)
        x, y, s = (v.ravel() for v in sv.get_state())
        wz = sv.get_bound_state()
        return dict(st=st, x=x, y=y, s=s, w=None if wz is None else wz[0].ravel(), z=None if wz is None else wz[1].ravel(),
                    hist=sv.history(), schedule=sv.schedule(), factor=sv.factor, refine=sv.refine_info())


def check_solve(cell, name, r):
    A, b, c, g, u, xs, ys = Q.problem(name)
    ref = Q.host_loop(name)
    st = r["st"]
    assert st["status"] == 1, (cell, st)
    assert abs(st["iterations"] - ref["iterations"]) <= 2, (cell, st["iterations"], ref["iterations"])
    rp, rd, gap = Q.stop_test_ld(A, b, c, g, u, r["x"], r["y"], r["s"], r["w"], r["z"])
    x_err = float(np.linalg.norm(r["x"] - xs) / np.linalg.norm(xs))
    obj_err = abs(st["objective"] - ref["obj_star"]) / abs(ref["obj_star"])
    host_obj_err = abs(ref["objective"] - ref["obj_star"]) / abs(ref["obj_star"])
    print("OBS %s iterations %d (host %d) rp %.3e rd %.3e gap %.3e x_err %.3e (host %.3e) obj_err %.3e (host %.3e)"
          % (cell, st["iterations"], ref["iterations"], rp, rd, gap, x_err, ref["x_err"], obj_err, host_obj_err))
    assert rp <= 2 * Q.TOL and rd <= 2 * Q.TOL and gap <= 2 * Q.TOL, (cell, rp, rd, gap)
    assert x_err <= max(1e-9, 100 * ref["x_err"]), (cell, x_err, ref["x_err"])
    assert obj_err <= max(1e-9, 100 * host_obj_err), (cell, obj_err, host_obj_err)
    assert st["alpha_p"] == st["alpha_d"] and all(h["alpha_p"] == h["alpha_d"] and h["alpha_aff_p"] == h["alpha_aff_d"] for h in r["hist"])


SOLVES = [("300x700", False, {}), ("300x700bm", False, {}), ("200x520b", True, {"factor": "dense"}), ("200x520b", True, {"factor": "sparse"}),
          ("2560x5120", False, {})]


@pytest.mark.parametrize("name,as_sparse,kw", SOLVES, ids=["%s%s" % (c[0], "-" + c[2]["factor"] if c[2] else "") for c in SOLVES])
def test_whole_solve(name, as_sparse, kw):
    r = _solve(name, as_sparse, **kw)
    assert r["schedule"]["fused_small"] == 0
    if kw:
        assert r["factor"] == kw["factor"]
    if name == "2560x5120":
        assert r["schedule"]["fused_factor"] == 1 and r["schedule"]["blocks"] == 20, r["schedule"]
    check_solve("%s/%s" % (name, kw.get("factor", "dense-ingest")), name, r)


def test_solve_front_end_small_sparse_problem_just_works():
    """solve(A_sparse_with_50_rows, ..., quad=g): the Python handle sets the term before A, so the multi-kernel path serves it."""
    A, b, c, g, u, xs, ys = workloads.separable_qp(50, 130, 5, bounded=True, mixed=True)
    x, y, s, info = ipm.solve_with_info(sparse.csc_matrix(A), b, c, ub=u, quad=g, tol=Q.TOL)
    ref = Q.solve64(A, b, c, g, u, tol=Q.TOL)
    assert info["status"] == 1 and info["quadratic"] == int((g > 0).sum()) and abs(info["iterations"] - ref["iterations"]) <= 2
    host_err = float(np.linalg.norm(ref["x"] - xs) / np.linalg.norm(xs))
    assert np.linalg.norm(x.ravel() - xs) / np.linalg.norm(xs) <= max(1e-9, 100 * host_err)
    assert ipm.solve_with_info(sparse.csc_matrix(A), b, c, ub=u, tol=Q.TOL, max_iter=3)[3]["quadratic"] == 0


def test_refined_solve_agrees():
    plain, refined = _solve("300x700bm"), _solve("300x700bm", refine=2)
    assert refined["st"]["status"] == 1 and refined["refine"].k == 2 and refined["refine"].solves > 0
    assert abs(refined["st"]["objective"] - plain["st"]["objective"]) <= 1e-8 * abs(plain["st"]["objective"])


def test_dense_column_split_solve_agrees():
    A, b, c, cols = workloads.block_angular_lp(400, 50, 8, seed=1)
    g = Q.quad_diagonal(A.shape[1], 7)
    out = []
    for kw in ({}, {"dense_cols": cols}):
        x, y, s, info = ipm.solve_with_info(A, b.ravel(), c.ravel(), factor="sparse", quad=g, tol=Q.TOL, **kw)
        assert info["status"] == 1 and info["factor_path"] == "sparse" and info["quadratic"] == int((g > 0).sum())
        out.append(info)
    unsplit, split = out
    assert unsplit["dense_cols"] is None and split["dense_cols"]["k"] == 8 and split["dense_cols"]["corrections"] > 0
    assert abs(split["objective"] - unsplit["objective"]) <= 1e-8 * abs(unsplit["objective"])


# ---- 3. invariants ----------------------------------------------------------------------------------------------------------
def _bits(sv):
    out = [v.tobytes() for v in sv.get_state()]
    wz = sv.get_bound_state()
    return out + ([] if wz is None else [v.tobytes() for v in wz])


def _record_bytes(records):
    """Statistics or history records as bytes: bit for bit, and a NaN equals itself."""
    return np.array([[float(r[k]) for k in sorted(r) if k != "solve_ms"] for r in records]).tobytes()


def _run(name, quad="problem", after=None, max_iter=5000, **kw):
    """A fresh handle on that problem -> (statistics, history, the state's bytes).  quad: the constructor's; after(sv): before the start."""
    A, b, c, g, u, xs, ys = Q.problem(name)
    with ipm.IpmSolver(A, b, c, ub=u, quad=g if isinstance(quad, str) else quad, **kw) as sv:
        if after:
            after(sv)
        sv.init_state(1.0)
        st = sv.solve(tol=Q.TOL, max_iter=max_iter)
        hist = sv.history()
        return st, (len(hist), _record_bytes([st]), _record_bytes(hist)), _bits(sv)


def test_bitwise_repeat():
    a, b = _run("300x700bm"), _run("300x700bm")
    assert a[0]["status"] == 1 and a[1:] == b[1:]


@pytest.mark.parametrize("name", ["300x700", "300x700bm"])
def test_clearing_restores_the_lp(name):
    n = Q.problem(name)[2].shape[0]
    never = _run(name, quad=None, max_iter=12)
    assert never[1][0] > 0
    for how in (lambda sv: sv.set_quadratic(None), lambda sv: sv.set_quadratic(np.zeros(n))):
        def clear(sv, how=how):
            assert sv.quadratic_nonzeros() > 0
            how(sv)
            assert sv.quadratic_nonzeros() == 0 and not sv.quadratic().any()
        assert _run(name, after=clear, max_iter=12)[1:] == never[1:]
    assert _run(name, max_iter=12)[1] != never[1]                          # (and the term does change the trajectory)


def test_independent_of_check_every():
    a, b = _run("300x700bm", check_every=1), _run("300x700bm", check_every=7)
    assert a[0]["status"] == 1 and a[1:] == b[1:]


@pytest.mark.parametrize("name", ["300x700bm"])
def test_independent_of_what_device_memory_held(name, monkeypatch):
    """The rule of tests/test_gpu_residue.py for the handle's new allocation: with every allocation of the library filled with 0x00 or
    0xFF bytes (NaN as doubles) before its first use, the solve is the one of an unfilled handle, bit for bit."""
    plain = _run(name)
    for fill in ("0", "255"):
        monkeypatch.setenv("IPM_TEST_ALLOC_FILL", fill)
        assert _run(name)[1:] == plain[1:], fill


def _badly_scaled(name, seed):
    """The problem with rows and columns times 10^U(-3, 3) (not powers of two) and g over the column factors squared: the same QP."""
    A, b, c, g, u, xs, ys = Q.problem(name)
    rng = np.random.default_rng(seed)
    dr, dc = 10.0 ** rng.uniform(-3, 3, A.shape[0]), 10.0 ** rng.uniform(-3, 3, A.shape[1])
    return dr[:, None] * A * dc[None, :], dr * b, dc * c, g * dc * dc, (None if u is None else u / dc)


@pytest.mark.parametrize("order", ["before", "after"])
@pytest.mark.parametrize("name", ["300x700", "300x700bm"])
def test_equilibration_equals_the_prescaled_problem(name, order):
    """The rule of tests/test_gpu_equilibrate.py: scale="ruiz" given g is bit-identical, after unscaling, to an unscaled handle given
    the host-prescaled (R A C, R b, C c, u / C, g C^2) -- with g set before the scaling (the constructor) and after it."""
    A, b, c, g, u = _badly_scaled(name, 11)
    er, ec, changed = EO.ruiz(A, 16)
    assert 0 < changed < 16
    R, Cc = EO.factors(er, ec)
    A2, b2, c2, u2 = EO.prescale(A, b, c, u, er, ec)
    g2 = g * Cc * Cc
    out = []
    for scaled in (True, False):
        args, ub, gg = ((A, b, c), u, g) if scaled else ((A2, b2, c2), u2, g2)
        with ipm.IpmSolver(*args, ub=ub, scale="ruiz" if scaled else None, quad=gg if (order == "before" or not scaled) else None) as sv:
            if scaled:
                assert np.array_equal(sv.scaling()[1], Cc) and sv.scale_info["passes"] == changed
                if order == "after":
                    sv.set_quadratic(gg)
            assert np.array_equal(sv.quadratic(), gg)                      # the getter: the caller's units, exactly
            sv.init_state(1.0)
            st = sv.solve(tol=Q.TOL, max_iter=40)
            out.append((st, sv.history(), sv.get_state(), sv.get_bound_state()))
    (st1, h1, (x1, y1, s1), wz1), (st2, h2, (x2, y2, s2), wz2) = out
    for k in ("status", "iterations", "objective", "rp_norm", "rd_norm", "gap", "b_norm", "c_norm", "alpha_p", "alpha_d"):
        assert st1[k] == st2[k], (k, st1[k], st2[k])
    assert st1["iterations"] > 0 and _record_bytes(h1) == _record_bytes(h2)
    Rc, Cv = R.reshape(-1, 1), Cc.reshape(-1, 1)
    assert np.array_equal(x1, Cv * x2) and np.array_equal(y1, Rc * y2) and np.array_equal(s1, s2 / Cv)
    if u is not None:
        assert np.array_equal(wz1[0], Cv * wz2[0]) and np.array_equal(wz1[1], wz2[1] / Cv)


def test_new_A_returns_the_term_to_the_callers_units():
    A, b, c, g, u = _badly_scaled("300x700", 12)
    with ipm.IpmSolver(A, b, c, scale="ruiz", quad=g) as sv:
        assert sv.scale_info["passes"] > 0 and np.array_equal(sv.quadratic(), g)
        sv._check(sv._lib.ipm_set_A_dense(sv._h, C.c_void_p(A.ctypes.data), sv.n, 0))
        assert np.all(sv.scaling()[1] == 1.0) and np.array_equal(sv.quadratic(), g) and sv.quadratic_nonzeros() == int((g > 0).sum())


# ---- 4. refusals and arguments ----------------------------------------------------------------------------------------------
def _small_problem():
    A, b, c, g, u, xs, ys = workloads.separable_qp(50, 130, 5)
    return sparse.csc_matrix(A), b, c, g


def test_bad_entries_are_rejected_and_the_old_term_is_kept():
    A, b, c, g, u, xs, ys = Q.problem("300x700")
    with ipm.IpmSolver(A, b, c, quad=g) as sv:
        for bad in (np.nan, np.inf, -1.0):
            gb = g.copy()
            gb[17] = bad
            with pytest.raises(ValueError):                                # the host check
                sv.set_quadratic(gb)
            assert sv._lib.ipm_set_quadratic(sv._h, _dptr(gb)) == _lib.ERR_INVALID_INPUT      # the library's own
            assert b"g[17]" in sv._lib.ipm_last_error(sv._h)
            assert np.array_equal(sv.quadratic(), g) and sv.quadratic_nonzeros() == int((g > 0).sum())
        with pytest.raises(ValueError):
            sv.set_quadratic(g[:-1])
        assert np.array_equal(sv.quadratic(), g)


def test_small_path_in_both_orders():
    A, b, c, g = _small_problem()
    with ipm.IpmSolver(A, b, c) as sv:                                     # A first: the one-workgroup path is taken ...
        assert sv.schedule()["fused_small"] == 1
        with pytest.raises(ipm.IpmError, match="before A") as ei:          # ... and a term then is refused
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
        sv.set_quadratic(None)                                             # clearing is always accepted
        sv.set_quadratic(np.zeros(sv.n))
        sv.init_state(1.0)
        assert sv.solve(tol=Q.TOL, max_iter=3)["iterations"] > 0           # and the handle stays usable
    with ipm.IpmSolver(A, b, c, quad=g) as sv:                             # the term first: never the small path
        assert sv.schedule()["fused_small"] == 0 and sv.quadratic_nonzeros() == int((g > 0).sum())


def test_lockstep_handle_refuses():
    A, b, c, g, u, xs, ys = Q.problem("200x520b")
    with ipm.IpmSolver(sparse.csc_matrix(A), b, c, lockstep=True, factor="dense") as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_LOCKSTEP") as ei:
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
        sv.set_quadratic(None)                                             # clearing is always accepted


def test_detect_handle_refuses():
    A, b, c, g, u, xs, ys = Q.problem("300x700")
    with ipm.IpmSolver(A, b, c, detect_infeasibility=True) as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_DETECT_INFEASIBILITY") as ei:
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
        sv.set_quadratic(np.zeros(sv.n))


def test_centrality_correctors_in_both_orders():
    A, b, c, g, u, xs, ys = Q.problem("300x700")
    with ipm.IpmSolver(A, b, c, correctors=2) as sv:                       # rounds first
        with pytest.raises(ipm.IpmError, match="centrality correctors") as ei:
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0 and sv.correctors == 2
        sv.set_correctors(0)
        sv.set_quadratic(g)                                                # the way out the message names
        assert sv.quadratic_nonzeros() == int((g > 0).sum())
    with ipm.IpmSolver(A, b, c, quad=g) as sv:                             # the term first
        with pytest.raises(ipm.IpmError, match="quadratic term") as ei:
            sv.set_correctors(1)
        assert ei.value.code == -1 and sv.correctors == 0 and sv.corrector_info()["k"] == 0
        sv.set_correctors(0)
        sv.set_quadratic(None)
        sv.set_correctors(1)                                               # without the term the rounds are accepted again
        assert sv.correctors == 1


def test_mehrotra_start_ignores_the_term():
    A, b, c, g, u, xs, ys = Q.problem("300x700bm")
    states = []
    for quad in (None, g):
        with ipm.IpmSolver(A, b, c, ub=u, quad=quad) as sv:
            sv.init_state_mehrotra()
            states.append(_bits(sv))
    assert states[0] == states[1]
