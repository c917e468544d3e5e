"""Free columns with curvature on the device (ipm_set_free_columns) and the factor-model QP built on them
(solve_factor_qp): min c.x + 1/2 x.(diag(g) + F F^T) x, A x = b, 0 <= x (<= u).

1. One iteration against the longdouble oracle of tests/free_qp_oracle.py, element by element: r_c, d, v, q (ipm_debug_get_column_vector),
   both directions, the step lengths, mu, sigma (which carries mu_aff), the updated state, the statistics and the history record, and
   s == ds == 0 exactly on the free columns.  The cells are the smallest at which the fourteen Free kernels (csrc/vector_ops.h) can
   go wrong: 1 barrier column + 1 free column with m = 1; free columns at j = 0, 255, 256, n - 1 of 40 x 600 (both sides of a
   VBLK = 256 block edge, both ends), plain and bounded, with x = 0 and x < 0 on two of them; free columns between bounded ones, one
   beside a column 1e-2 from its bound; all but one column free; 130 x 300 as CSC on the envelope factor and on the sparse factor,
   plain and bounded; 8 x 16500 as CSC (n > MAXPART VBLK = 16384: the grid-stride loop's second trip) with free columns in both trips.
2. iterate(3) equals three iterate(1), bit for bit.
3. Whole solves of workloads.factor_qp through solve_factor_qp against the float64 host loop of free_qp_oracle.
4. Invariants: bitwise repeat; set-then-cleared equals never-set; the order of the setter against A and ipm_set_quadratic;
   check_every; what device memory held before; scale="ruiz" against the host-prescaled problem; refine=2.
5. The state seams and every refusal the library decides, in both orders of the calls.

Bounds of part 1: test_gpu_iteration_edges._bound, unchanged (100 x the maxima observed there, floor 1e-12); r_c, d, v, q, which
that file does not read, get its floor, 1e-12 (tests/test_free_qp_host.py holds the float64 restatement to the oracle under it).
Bounds of part 3: the device's iteration count EQUALS the host loop's; ||x - x*|| / ||x*|| against the constructed optimum by the rule
of test_gpu_qp.check_solve, max(1e-9, 100 x the host loop's own error), y alike; the stop test's three inequalities recomputed in
longdouble on the augmented problem hold with its factor 2; t = F^T x to the primal residual that stop test allows,
2 tol (1 + ||(b, u_U)||); info["objective"] is recomputed from x with the same expression: 1e-13.

Observed maxima on MI355X: see OBSERVED_FREE / OBSERVED_SOLVES below.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import workloads

import equilibrate_oracle as EO
import free_qp_oracle as FO
import iteration_oracle as IO
import qp_oracle as Q
from test_gpu_iteration_edges import FLOOR, OBSERVED, _assert_all, _bound, _srel

pytestmark = pytest.mark.gpu

# the maxima of the first run of this file on an MI355X, over the cells of part 1, for the record (the bounds are _bound's and FLOOR, not
# multiples of these; every quantity stayed under its bound on that run, so no bound was replaced).  The largest: q 5.7e-15, dxa 4.9e-15,
# dx 4.5e-15, v 3.8e-15 at sparse/8x16500; ds 3.2e-15, s 2.6e-15 at 5x50-all-but-one; dz 2.6e-15, dw 2.4e-15 at 40x600b-interleaved.
OBSERVED_FREE = {"dxa": 4.9e-15, "dsa": 3.4e-15, "ATdya": 3.4e-15, "dya": 3.4e-15, "dx": 4.5e-15, "ds": 3.2e-15, "dw": 2.4e-15, "dz": 2.6e-15,
                 "ATdy": 1.4e-16, "dy": 1.8e-15, "x": 1.6e-15, "s": 2.6e-15, "w": 6.8e-16, "z": 7.8e-16, "ATy": 1.7e-15, "y": 1.5e-15,
                 "alpha_aff_p": 1.5e-15, "alpha_aff_d": 1.5e-15, "alpha_p": 2.1e-15, "alpha_d": 2.1e-15, "mu": 4.7e-16, "mu_aff": 5.2e-16,
                 "sigma": 1.8e-15, "gap": 4.3e-16, "objective": 1.4e-16, "rp_norm": 4.0e-16, "rd_norm": 1.6e-16, "rc": 2.4e-16, "d": 5.7e-17,
                 "v": 3.8e-15, "q": 5.7e-15}
# whole solves: (iterations = the host loop's, x error, the host loop's x error)
OBSERVED_SOLVES = {"1x64k8b": (11, 4.471e-11, 4.471e-11), "40x130k8b": (12, 3.745e-12, 3.745e-12), "300x700k64": (12, 2.537e-12, 2.537e-12),
                   "200x520k16": (12, 1.704e-12, 1.704e-12), "2560x5120k64": (13, 4.534e-13, 4.539e-13)}
TOL = FO.TOL


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _bound_free(k):
    return _bound(k) if k.split(".")[-1] in OBSERVED else FLOOR


# ---- 1. one iteration against the oracle ------------------------------------------------------------------------------------
def check_free_iteration(cell, sv, case, g, free, o):
    AT = case.A.T
    fm = FO.free_mask(free, case.n)
    e = {}

    def vec(k, got, want):
        e[k] = IO.rel(got, want)

    def scal(k, got, want):
        e[k] = _srel(got, want)

    assert np.array_equal(sv.free_columns(), free) and np.array_equal(sv.quadratic(), g)
    sv.set_state(*case.state())
    assert np.all(sv.get_state()[2].ravel()[fm] == 0) and np.any(case.s[fm] != 0)       # set_state stores s = 0 there, whatever is passed
    dxa, dya, dsa = sv.newton_direction(False)
    st = dict(sv.stats)
    vec("aff.rc", sv.debug_column_vector("rc"), o["rc"]); vec("aff.d", sv.debug_column_vector("d"), o["theta"])
    vec("aff.v", sv.debug_column_vector("v"), o["va"]); vec("aff.q", sv.debug_column_vector("q"), o["qa"])
    assert np.all(sv.debug_column_vector("q")[fm] == 0) and np.array_equal(sv.debug_column_vector("d")[fm], 1.0 / g[fm])
    vec("dxa", dxa, o["dxa"]); vec("dsa", dsa, o["dsa"]); vec("ATdya", AT @ dya.ravel(), o["atdya"]); vec("dya", dya, o["dya"])
    assert np.all(dsa.ravel()[fm] == 0)
    scal("aff.alpha_aff_p", st["alpha_aff_p"], o["alpha_aff_p"]); scal("aff.alpha_aff_d", st["alpha_aff_d"], o["alpha_aff_d"])
    scal("aff.mu", st["mu"], o["mu"])
    assert st["alpha_aff_p"] == st["alpha_aff_d"]
    dx, dy, ds = sv.newton_direction(True)
    st = dict(sv.stats)
    vec("cor.v", sv.debug_column_vector("v"), o["v"]); vec("cor.q", sv.debug_column_vector("q"), o["q"])
    assert np.all(sv.debug_column_vector("q")[fm] == 0)
    vec("dx", dx, o["dx"]); vec("ds", ds, o["ds"]); vec("ATdy", AT @ dy.ravel(), o["atdy"]); vec("dy", dy, o["dy"])
    assert np.all(ds.ravel()[fm] == 0)
    scal("cor.mu", st["mu"], o["mu"]); scal("cor.sigma", st["sigma"], o["sigma"]); scal("cor.mu_aff", st["mu_aff"], o["mu_aff"])

    sv.set_state(*case.state())
    st = sv.iterate(1)
    x, y, s = sv.get_state()
    vec("x", x, o["xn"]); vec("s", s, o["sn"]); vec("ATy", AT @ y.ravel(), o["atyn"]); vec("y", y, o["yn"])
    assert np.all(s.ravel()[fm] == 0)
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
        scal("hist." + k, h[k], o[k])
    e["hist.rp_norm"] = IO.residual_rel(h["rp_norm"], o["rp_norm"], o["b_norm"])
    e["hist.rd_norm"] = IO.residual_rel(h["rd_norm"], o["rd_norm"], o["c_norm"])
    assert h["alpha_p"] == st["alpha_p"] and h["alpha_d"] == st["alpha_d"]
    assert st["alpha_p"] == st["alpha_d"] and h["alpha_aff_p"] == h["alpha_aff_d"]                 # ONE step length, exactly
    # the free columns are really outside mu: the pair count n (+ |U|) would give a mu off by the ratio of the counts
    pairs = case.n - int(fm.sum()) + int(case.U.sum())
    assert abs(h["mu"] * pairs - h["gap"]) <= 1e-14 * h["gap"] and pairs < case.n + int(case.U.sum())
    _assert_all(cell, e, {k: _bound_free(k) for k in e})


CELLS = [("1x2", False, None), ("40x600", False, None), ("40x600b", False, None), ("40x600b-interleaved", False, None),
         ("5x50-all-but-one", False, None), ("sparse/130x300", True, "dense"), ("sparse/130x300", True, "sparse"),
         ("sparse/130x300b", True, "dense"), ("sparse/130x300b", True, "sparse"), ("sparse/8x16500", True, None)]
CELL_IDS = ["%s%s" % (c[0], "-" + c[2] if c[2] else "") for c in CELLS]


def _cell_solver(name, as_sparse, factor, **kw):
    case, g, free = FO.get(name)
    A = sparse.csc_matrix(case.A) if as_sparse else case.A
    if factor is not None:
        kw["factor"] = factor
    return ipm.IpmSolver(A, case.b, case.c, ub=case.ub(), quad=g, free=free, **kw)


@pytest.mark.parametrize("name,as_sparse,factor", CELLS, ids=CELL_IDS)
def test_one_iteration(name, as_sparse, factor):
    case, g, free = FO.get(name)
    with _cell_solver(name, as_sparse, factor) as sv:
        sch = sv.schedule()
        assert sch["fused_small"] == 0 and sv.sparse == as_sparse and sv.bounded == int(case.U.sum())
        if factor == "sparse":
            assert sv.factor == "sparse" and sv.factor_info()["panels"] >= 1
        elif factor == "dense":
            assert sv.factor == "dense" and sch["blocks"] == (case.m + 127) // 128
        check_free_iteration("%s/factor=%s" % (name, factor), sv, case, g, free, FO.oracle(name))


# ---- 2. iterate(3) == 3 x iterate(1) ----------------------------------------------------------------------------------------
def _bits(sv):
    out = [v.tobytes() for v in sv.get_state()]
    wz = sv.get_bound_state()
    return out + ([] if wz is None else [v.tobytes() for v in wz])


def _record_bytes(records):
    """Statistics or history records as bytes: bit for bit, and a NaN equals itself."""
    return np.array([[float(r[k]) for k in sorted(r) if k not in ("solve_ms", "k", "iterations")] for r in records]).tobytes()


@pytest.mark.parametrize("name,as_sparse,factor", [("40x600b", False, None), ("sparse/130x300b", True, "sparse")], ids=["dense", "sparse-factor"])
def test_three_steps_at_once_equal_three_single_steps(name, as_sparse, factor):
    case, g, free = FO.get(name)
    out = []
    for steps in ((3,), (1, 1, 1)):
        with _cell_solver(name, as_sparse, factor) as sv:
            sv.set_state(*case.state())
            for k in steps:
                st = sv.iterate(k)
            out.append((_bits(sv), _record_bytes([st])))
            assert np.all(np.isfinite(sv.get_state()[0]))
    assert out[0] == out[1]


# ---- 3. whole solves --------------------------------------------------------------------------------------------------------
SOLVES = [("1x64k8b", False, {}), ("40x130k8b", False, {}), ("300x700k64", False, {}), ("200x520k16", True, {"factor": "dense"}),
          ("200x520k16", True, {"factor": "sparse"}), ("2560x5120k64", False, {})]
SOLVE_IDS = ["%s%s" % (c[0], "-" + c[2]["factor"] if c[2] else "") for c in SOLVES]


def check_factor_solve(cell, name, x, y, s, info):
    A, b, c, g, F, u, xs, ys = FO.problem(name)
    ref = FO.host_loop(name)
    m, n = A.shape
    k = F.shape[1]
    x, y, s = x.ravel(), y.ravel(), s.ravel()
    assert info["status"] == 1, (cell, info["status"])
    assert info["factors"] == k and info["free"] == k and info["quadratic"] == n + k and info["quadratic_path"] == "multi-kernel"
    x_err = float(np.linalg.norm(x - xs) / np.linalg.norm(xs))
    y_err = float(np.linalg.norm(y - ys) / np.linalg.norm(ys))
    ftx = F.T @ x
    t_gap = float(np.linalg.norm(info["t"] - ftx))
    A_, b_, c_, g_, u_, free = ipm.factor_qp_form(A, b, c, g, F, u)
    xa, ya = np.concatenate([x, info["t"]]), np.concatenate([y, info["y_factor"]])
    sa = np.concatenate([s, np.zeros(k)])
    pad = (lambda v: None if v is None else np.concatenate([np.asarray(v).ravel(), np.zeros(k)]))
    rp, rd, gap = Q.stop_test_ld(A_, b_, c_, g_, u_, xa, ya, sa, pad(info.get("w")), pad(info.get("z")))
    obj = float(c @ x + 0.5 * (g * x) @ x + 0.5 * (ftx @ ftx))
    print("OBS %s iterations %d (host %d) rp %.3e rd %.3e gap %.3e x_err %.3e (host %.3e) y_err %.3e (host %.3e) t_gap %.3e obj_rel %.3e"
          % (cell, info["iterations"], ref["iterations"], rp, rd, gap, x_err, ref["x_err"], y_err, ref["y_err"], t_gap,
             abs(obj - ref["obj_star"]) / abs(ref["obj_star"])))
    assert info["iterations"] == ref["iterations"], (cell, info["iterations"], ref["iterations"])
    assert rp <= 2 * TOL and rd <= 2 * TOL and gap <= 2 * TOL, (cell, rp, rd, gap)
    assert x_err <= max(1e-9, 100 * ref["x_err"]), (cell, x_err, ref["x_err"])
    assert y_err <= max(1e-9, 100 * ref["y_err"]), (cell, y_err, ref["y_err"])
    bu = np.sqrt(b_ @ b_ + (0.0 if u is None else float(u[np.isfinite(u)] @ u[np.isfinite(u)])))          # ||(b, u_U)||, the stop test's norm
    assert t_gap <= 2 * TOL * (1 + bu), (cell, t_gap)
    assert abs(info["objective"] - obj) <= 1e-13 * abs(obj), (cell, info["objective"], obj)
    assert abs(info["objective"] - ref["obj_star"]) <= 1e-7 * abs(ref["obj_star"])
    assert info["alpha_p"] == info["alpha_d"]
    assert np.all(s >= 0) and np.all(x > 0)


@pytest.mark.parametrize("name,as_sparse,kw", SOLVES, ids=SOLVE_IDS)
def test_whole_solve(name, as_sparse, kw):
    A, b, c, g, F, u, xs, ys = FO.problem(name)
    x, y, s, info = ipm.solve_factor_qp(sparse.csc_matrix(A) if as_sparse else A, b, c, F, g=g, ub=u, tol=TOL, **kw)
    assert x.shape == (A.shape[1], 1) and y.shape == (A.shape[0], 1) and s.shape == x.shape and info["t"].shape == (F.shape[1],)
    if kw:
        assert info["factor_path"] == kw["factor"]
    check_factor_solve("%s/%s" % (name, kw.get("factor", "dense-ingest")), name, x, y, s, info)


def _augmented(name):
    A, b, c, g, F, u, xs, ys = FO.problem(name)
    return ipm.factor_qp_form(A, b, c, g, F, u)


def test_the_large_dense_shape_takes_the_fused_launch():
    A_, b_, c_, g_, u_, free = _augmented("2560x5120k64")
    with ipm.IpmSolver(A_, b_, c_, ub=u_, quad=g_, free=free) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=TOL)
        sch = sv.schedule()
        assert sch["fused_factor"] == 1 and sch["fused_small"] == 0 and sch["blocks"] == 21, sch
        assert st["status"] == 1 and st["iterations"] == FO.host_loop("2560x5120k64")["iterations"]


# ---- 4. invariants ----------------------------------------------------------------------------------------------------------
def _run(name, quad="problem", free="problem", after=None, max_iter=5000, as_sparse=False, **kw):
    """A fresh handle on that problem's augmented form -> (statistics, (records, their bytes), the state's bytes).
    quad / free: the constructor's ("problem": the problem's own); after(sv): called before the start."""
    A_, b_, c_, g_, u_, fr = _augmented(name)
    with ipm.IpmSolver(sparse.csc_matrix(A_) if as_sparse else A_, b_, c_, ub=u_, quad=g_ if isinstance(quad, str) else quad,
                       free=fr if isinstance(free, str) else free, **kw) as sv:
        if after:
            after(sv)
        sv.init_state(1.0)
        st = sv.solve(tol=TOL, max_iter=max_iter)
        hist = sv.history()
        return st, (len(hist), _record_bytes([st]), _record_bytes(hist)), _bits(sv)


NAME = "40x130k8b"          # bounded, dense ingest; 300x700k64 for the plain kernels


@pytest.mark.parametrize("name", [NAME, "300x700k64"])
def test_bitwise_repeat(name):
    a, b = _run(name), _run(name)
    assert a[0]["status"] == 1 and a[1:] == b[1:]


@pytest.mark.parametrize("name", [NAME, "300x700k64"])
def test_set_then_cleared_equals_never_set(name):
    never = _run(name, free=None, max_iter=6)
    assert never[1][0] > 0
    for how in (lambda sv: sv.set_free(None), lambda sv: sv.set_free([]), lambda sv: sv._check(sv._lib.ipm_set_free_columns(sv._h, None, 3))):
        def clear(sv, how=how):
            assert sv.free_columns().shape[0] > 0
            how(sv)
            assert sv.free_columns().shape[0] == 0
        assert _run(name, after=clear, max_iter=6)[1:] == never[1:]
    assert _run(name, max_iter=6)[1] != never[1]                               # (and the set does change the trajectory)


@pytest.mark.parametrize("name", [NAME, "300x700k64"])
def test_order_of_the_setters(name):
    """The constructor sets g, then the free set, then A.  The set after A (and after g), and the set after A but BEFORE g, give the same
    solve bit for bit."""
    A_, b_, c_, g_, u_, fr = _augmented(name)
    ctor = _run(name)

    def after_A(sv):
        assert sv.free_columns().shape[0] == 0
        sv.set_free(fr)

    def before_g(sv):
        assert sv.quadratic_nonzeros() == 0
        sv.set_free(fr)
        sv.set_quadratic(g_)
    assert _run(name, free=None, after=after_A)[1:] == ctor[1:]
    assert _run(name, quad=None, free=None, after=before_g)[1:] == ctor[1:]
    assert ctor[0]["status"] == 1


def test_independent_of_check_every():
    a, b = _run(NAME, check_every=1), _run(NAME, check_every=7)
    assert a[0]["status"] == 1 and a[1:] == b[1:]


@pytest.mark.parametrize("name,as_sparse,kw", [(NAME, False, {}), ("200x520k16", True, {"factor": "sparse"})], ids=["dense", "sparse-factor"])
def test_independent_of_what_device_memory_held(name, as_sparse, kw, monkeypatch):
    """The rule of tests/test_gpu_residue.py for the handle's new allocation (the byte marks): with every allocation of the library
    filled with 0x00 or 0xFF bytes before its first use, the solve is the one of an unfilled handle, bit for bit."""
    plain = _run(name, as_sparse=as_sparse, **kw)
    assert plain[0]["status"] == 1
    for fill in ("0", "255"):
        monkeypatch.setenv("IPM_TEST_ALLOC_FILL", fill)
        assert _run(name, as_sparse=as_sparse, **kw)[1:] == plain[1:], fill


@pytest.mark.parametrize("name", [NAME, "300x700k64"])
def test_equilibration_equals_the_prescaled_problem(name):
    """The rule of tests/test_gpu_equilibrate.py: scale="ruiz" is bit-identical, after unscaling, to an unscaled handle given the
    host-prescaled (R A C, R b, C c, u / C, g C^2) with the same free set: the marks are scale-free."""
    A_, b_, c_, g_, u_, fr = _augmented(name)
    rng = np.random.default_rng(11)
    dr, dc = 10.0 ** rng.uniform(-3, 3, A_.shape[0]), 10.0 ** rng.uniform(-3, 3, A_.shape[1])
    A, b, c, g, u = dr[:, None] * A_ * dc[None, :], dr * b_, dc * c_, g_ * dc * dc, (None if u_ is None else u_ / dc)
    er, ec, changed = EO.ruiz(A, 16)
    assert 0 < changed < 16
    R, Cc = EO.factors(er, ec)
    A2, b2, c2, u2 = EO.prescale(A, b, c, u, er, ec)
    g2 = g * Cc * Cc
    out = []
    for scaled in (True, False):
        args, ub, gg = ((A, b, c), u, g) if scaled else ((A2, b2, c2), u2, g2)
        with ipm.IpmSolver(*args, ub=ub, scale="ruiz" if scaled else None, quad=gg, free=fr) as sv:
            if scaled:
                assert np.array_equal(sv.scaling()[1], Cc) and sv.scale_info["passes"] == changed
            assert np.array_equal(sv.free_columns(), fr)
            sv.init_state(1.0)
            st = sv.solve(tol=TOL, max_iter=40)
            out.append((st, sv.history(), sv.get_state(), sv.get_bound_state()))
    (st1, h1, (x1, y1, s1), wz1), (st2, h2, (x2, y2, s2), wz2) = out
    for k in ("status", "iterations", "objective", "rp_norm", "rd_norm", "gap", "b_norm", "c_norm", "alpha_p", "alpha_d"):
        assert st1[k] == st2[k], (k, st1[k], st2[k])
    assert st1["iterations"] > 0 and _record_bytes(h1) == _record_bytes(h2)
    Rc, Cv = R.reshape(-1, 1), Cc.reshape(-1, 1)
    assert np.array_equal(x1, Cv * x2) and np.array_equal(y1, Rc * y2) and np.array_equal(s1, s2 / Cv)
    assert np.all(s1.ravel()[fr] == 0)
    if u is not None:
        assert np.array_equal(wz1[0], Cv * wz2[0]) and np.array_equal(wz1[1], wz2[1] / Cv)


def test_refined_solve_agrees():
    A, b, c, g, F, u, xs, ys = FO.problem("300x700k64")
    plain = ipm.solve_factor_qp(A, b, c, F, g=g, ub=u, tol=TOL)[3]
    refined = ipm.solve_factor_qp(A, b, c, F, g=g, ub=u, tol=TOL, refine=2)[3]
    assert refined["status"] == 1 and refined["refine"].k == 2 and refined["refine"].solves > 0
    assert abs(refined["objective"] - plain["objective"]) <= 1e-8 * abs(plain["objective"])


def test_dense_column_split_solve_agrees():
    """The dense-column split of the sparse factor serves a handle with free columns: it reads only d."""
    A, b, c, cols = workloads.block_angular_lp(400, 50, 8, seed=1)
    n = A.shape[1]
    g = np.random.default_rng(3).uniform(0.1, 2.0, n)
    F = np.random.default_rng(4).standard_normal((n, 4)) / np.sqrt(n)
    out = []
    for kw in ({}, {"dense_cols": cols}):
        x, y, s, info = ipm.solve_factor_qp(A, b.ravel(), c.ravel(), F, g=g, factor="sparse", tol=TOL, **kw)
        assert info["status"] == 1 and info["factor_path"] == "sparse" and info["free"] == 4
        out.append(info)
    unsplit, split = out
    assert unsplit["dense_cols"] is None and split["dense_cols"]["k"] == 8 and split["dense_cols"]["corrections"] > 0
    assert abs(split["objective"] - unsplit["objective"]) <= 1e-8 * abs(unsplit["objective"])


# ---- 5. state seams and refusals ----------------------------------------------------------------------------------------------
def _handle(name=NAME, free="problem", quad="problem", **kw):
    A_, b_, c_, g_, u_, fr = _augmented(name)
    return ipm.IpmSolver(A_, b_, c_, ub=kw.pop("ub", u_), quad=g_ if isinstance(quad, str) else quad, free=fr if isinstance(free, str) else free, **kw), g_, fr


def test_state_seams():
    sv, g_, fr = _handle()
    with sv:
        sv.init_state(1.0)
        x, y, s = (v.ravel() for v in sv.get_state())
        assert np.all(s[fr] == 0) and np.all(x == 1) and np.all(np.delete(s, fr) == 1)
        sv.set_state(np.full(sv.n, 2.0), np.zeros(sv.m), np.full(sv.n, 3.0))
        x, y, s = (v.ravel() for v in sv.get_state())
        assert np.all(s[fr] == 0) and np.all(np.delete(s, fr) == 3) and np.all(x == 2)
        sv.set_free(fr[:2])                                                     # changed on a handle that holds a state
        assert np.array_equal(sv.free_columns(), fr[:2]) and np.all(sv.get_state()[2].ravel()[fr] == 0)
        sv.set_state(np.full(sv.n, 2.0), np.zeros(sv.m), np.full(sv.n, 3.0))
        sv.set_free(fr[1:4])                                                    # s goes to 0 on the NEW free columns; elsewhere it stays what was stored
        s = sv.get_state()[2].ravel()
        assert np.all(s[fr[1:4]] == 0) and s[fr[0]] == 0 and s[fr[4]] == 3      # (fr[0] was free when the state went in)
        sv.set_free(None)                                                       # cleared: the former free columns still hold s = 0 ...
        assert sv.free_columns().shape[0] == 0 and np.all(sv.get_state()[2].ravel()[fr[1:4]] == 0)
        sv.init_state(1.0)                                                      # ... so the caller sets a state anew, as the header says
        assert np.all(sv.get_state()[2] == 1)
        st = sv.iterate(2)
        assert st["iterations"] == 2 and np.all(np.isfinite(sv.get_state()[0])) and np.all(sv.get_state()[2] > 0)


def _refused(sv, code, word, call):
    rc = call()
    assert rc == code, (rc, sv._lib.ipm_last_error(sv._h))
    assert word.encode() in sv._lib.ipm_last_error(sv._h), sv._lib.ipm_last_error(sv._h)


def test_bad_indices_are_refused_and_the_set_is_kept():
    sv, g_, fr = _handle()
    with sv:
        lib, h = sv._lib, sv._h
        for idx, word in (([int(fr[0]), sv.n], "out of range"), ([-1], "out of range"), ([int(fr[0]), int(fr[1]), int(fr[0])], "duplicated")):
            a = np.array(idx, dtype=np.int32)
            _refused(sv, -1, word, lambda: lib.ipm_set_free_columns(h, _iptr(a), len(idx)))
            assert np.array_equal(sv.free_columns(), fr)
        _refused(sv, -1, "count", lambda: lib.ipm_set_free_columns(h, _iptr(fr), -2))
        k = C.c_int32(0)
        two = np.zeros(2, dtype=np.int32)
        assert lib.ipm_get_free_columns(h, _iptr(two), 2, C.byref(k)) == 0 and k.value == fr.shape[0] and np.array_equal(two, fr[:2])
        with pytest.raises(ValueError, match="out of range"):
            sv.set_free([sv.n])
        with pytest.raises(ValueError, match="twice"):
            sv.set_free([1, 1])


def test_column_without_curvature_in_both_orders():
    A_, b_, c_, g_, u_, fr = _augmented(NAME)
    j = int(fr[0])
    g0 = g_.copy()
    g0[j] = 0.0
    sv, _, _ = _handle(free=None, quad=g0)
    with sv:                                                                    # the term first
        with pytest.raises(ipm.IpmError, match="g = 0") as ei:
            sv.set_free(fr)
        assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
    sv, _, _ = _handle(free=None, quad=None)
    with sv:                                                                    # the set first
        sv.set_free(fr)
        sv.init_state(1.0)
        with pytest.raises(ipm.IpmError, match="without a quadratic term") as ei:          # no term ever came
            sv.iterate(1)
        assert ei.value.code == -1
        with pytest.raises(ipm.IpmError, match="free column") as ei:
            sv.set_quadratic(g0)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0 and np.array_equal(sv.free_columns(), fr)
        sv.set_quadratic(g_)
        assert sv.iterate(1)["iterations"] == 1
        for bad in (None, np.zeros(sv.n), g0):                                  # clearing or zeroing g on a free column
            assert sv._lib.ipm_set_quadratic(sv._h, None if bad is None else _dptr(bad)) == -1
            assert b"free column" in sv._lib.ipm_last_error(sv._h) and np.array_equal(sv.quadratic(), g_)
        sv.set_free(None)
        sv.set_quadratic(None)                                                  # the way out the message names


def test_finite_bound_in_both_orders():
    A_, b_, c_, g_, u_, fr = _augmented(NAME)
    ub = u_.copy()
    ub[fr[2]] = 5.0
    sv, _, _ = _handle()
    with sv:                                                                    # the set first
        _refused(sv, -1, "free column", lambda: sv._lib.ipm_set_bounds(sv._h, _dptr(ub)))
        assert sv.bounded == int(np.isfinite(u_).sum()) and np.array_equal(sv.free_columns(), fr)
        sv.init_state(1.0)
        assert sv.solve(tol=TOL)["status"] == 1                                 # the handle kept its bounds and stays usable
    sv, _, _ = _handle(free=None, ub=ub)
    with sv:                                                                    # the bound first
        with pytest.raises(ipm.IpmError, match="finite upper bound") as ei:
            sv.set_free(fr)
        assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
        sv.set_free(np.delete(fr, 2))


def test_no_pair_left_is_refused():
    A_, b_, c_, g_, u_, fr = _augmented("300x700k64")
    with ipm.IpmSolver(A_, b_, c_, quad=g_) as sv:
        every = np.arange(sv.n, dtype=np.int32)
        _refused(sv, -1, "no complementarity pair", lambda: sv._lib.ipm_set_free_columns(sv._h, _iptr(every), sv.n))
        sv.set_free(every[1:])                                                  # one pair is enough (test_one_iteration: all but one)


def test_lockstep_and_detect_handles_refuse():
    A_, b_, c_, g_, u_, fr = _augmented("200x520k16")
    with ipm.IpmSolver(sparse.csc_matrix(A_), b_, c_, lockstep=True, factor="dense") as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_LOCKSTEP") as ei:
            sv.set_free(fr)
        assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
        sv.set_free(None)                                                       # clearing is always accepted
    with ipm.IpmSolver(A_, b_, c_, detect_infeasibility=True) as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_DETECT_INFEASIBILITY") as ei:
            sv.set_free(fr)
        assert ei.value.code == -1
    with ipm.IpmSolver(A_, b_, c_, quad=g_, free=fr) as sv:                     # centrality correctors: the quadratic handle's refusal
        with pytest.raises(ipm.IpmError, match="quadratic term"):
            sv.set_correctors(1)


def test_small_path_in_both_orders():
    A, b, c, g, u, xs, ys = workloads.separable_qp(50, 130, 5)
    A = sparse.csc_matrix(A)
    for kw in ({}, {"quad": g, "quad_small": True}):
        with ipm.IpmSolver(A, b, c, **kw) as sv:                                # A first: the one-workgroup path is taken ...
            assert sv.schedule()["fused_small"] == 1
            with pytest.raises(ipm.IpmError, match="before A") as ei:           # ... and a free set then is refused
                sv.set_free([3])
            assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
            sv.set_free(None)
            sv.init_state(1.0)
            assert sv.solve(tol=TOL, max_iter=3)["iterations"] > 0              # and the handle stays usable
    with ipm.IpmSolver(A, b, c, quad=g, quad_small=True, free=[3]) as sv:       # the set first: never the small path, flag or not
        assert sv.schedule()["fused_small"] == 0 and sv.free_columns().tolist() == [3]
        sv.init_state(1.0)
        assert sv.solve(tol=TOL)["status"] == 1


def test_mehrotra_start_is_refused():
    sv, g_, fr = _handle()
    with sv:
        with pytest.raises(ipm.IpmError, match="ipm_init_state_mehrotra") as ei:
            sv.init_state_mehrotra()
        assert ei.value.code == -1
        sv.set_free(None)
        sv.init_state_mehrotra()                                                # without the set the start runs
