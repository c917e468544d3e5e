"""LP free columns on the device (ipm_set_free_lp_columns): free variables of a linear program served natively by
proximal-point regularisation of the free block.

1. One iteration against the longdouble oracle of tests/free_lp_oracle.py, element by element: r_c, d, v, q
   (ipm_debug_get_column_vector), both directions, the four step lengths, mu, mu_aff, sigma, the updated state, the history record,
   s == ds == 0 exactly on the free columns and d_j == 1 / rho exactly.  The cells are those of tests/test_gpu_free_qp.py: 1 barrier
   + 1 free column with m = 1; free columns at j = 0, 255, 256, n - 1 of 40 x 600 (both sides of a VBLK = 256 block edge, both
   ends), plain and bounded, with x = 0 and x < 0 on two of them; free columns between bounded ones, one beside a column 1e-2 from
   its bound; all but one column free; 130 x 300 as CSC on the envelope factor and on the sparse factor, plain and bounded;
   8 x 16500 as CSC (the grid-stride loop's second trip).  These run at rho = free_lp_oracle.ITER_RHO = 0.25, which says why: the
   comparison is of arithmetic at 1e-12, and cond(A Theta A^T) eps bounds it from below at 1e-8 for rho = 1e-8 in ANY float64 code.
   d_j == 1 / rho is asserted at the default rho too.
2. iterate(3) equals three iterate(1), bit for bit; the device Mehrotra start against IpmSolver.mehrotra_start restated for the
   set (the rule of tests/test_gpu_mehrotra_start.py: 10 x the host restatement's own error against dense NumPy, floor 1e-13),
   plain, bounded and at the degenerate fallback.
3. Whole solves of workloads.free_lp at the DEFAULT rho against the float64 host loop of free_lp_oracle, by the rule of
   test_gpu_qp.check_solve: status 1, iterations within +-2, the stop test's residuals recomputed in longdouble <= 2 tol,
   x_err <= max(1e-9, 100 x the host loop's); dependent=True: objective and residuals only.
4. Invariants: bitwise repeat; set-then-cleared equals never-set; the order of the setters; check_every; what device memory held
   before; scale="ruiz" against the host-prescaled problem (rho in the handle's units), bitwise; refine=2; the dense-column split.
5. The state seams, every refusal in both orders of the calls, and new_interior_sparse(bounds="native", free="native").
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import general_form, workloads

import equilibrate_oracle as EO
import free_lp_oracle as FL
import iteration_oracle as IO
import qp_oracle as Q
from test_gpu_iteration_edges import FLOOR, OBSERVED, _assert_all, _bound, _srel

pytestmark = pytest.mark.gpu
TOL = FL.TOL
RHO = FL.ITER_RHO


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _bound_free(k):
    return _bound(k) if k.split(".")[-1] in OBSERVED else FLOOR


# ---- 1. one iteration against the oracle ------------------------------------------------------------------------------------
def check_free_lp_iteration(cell, sv, case, free, o):
    AT = case.A.T
    fm = FL.free_mask(free, case.n)
    e = {}

    def vec(k, got, want):
        e[k] = IO.rel(got, want)

    def scal(k, got, want):
        e[k] = _srel(got, want)

    idx, rho = sv.free_lp_columns()
    assert np.array_equal(idx, free) and rho == RHO and sv.quadratic_nonzeros() == 0 and sv.free_columns().shape[0] == 0
    sv.set_state(*case.state())
    assert np.all(sv.get_state()[2].ravel()[fm] == 0) and np.any(case.s[fm] != 0)       # set_state stores s = 0 there, whatever is passed
    dxa, dya, dsa = sv.newton_direction(False)
    st = dict(sv.stats)
    vec("aff.rc", sv.debug_column_vector("rc"), o["rc"]); vec("aff.d", sv.debug_column_vector("d"), o["theta"])
    vec("aff.v", sv.debug_column_vector("v"), o["va"]); vec("aff.q", sv.debug_column_vector("q"), o["qa"])
    assert np.all(sv.debug_column_vector("q")[fm] == 0) and np.all(sv.debug_column_vector("d")[fm] == 1.0 / RHO)
    vec("dxa", dxa, o["dxa"]); vec("dsa", dsa, o["dsa"]); vec("ATdya", AT @ dya.ravel(), o["atdya"]); vec("dya", dya, o["dya"])
    assert np.all(dsa.ravel()[fm] == 0)
    scal("aff.alpha_aff_p", st["alpha_aff_p"], o["alpha_aff_p"]); scal("aff.alpha_aff_d", st["alpha_aff_d"], o["alpha_aff_d"])
    scal("aff.mu", st["mu"], o["mu"])
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
    # the free columns are really outside mu: the pair count n (+ |U|) would give a mu off by the ratio of the counts
    pairs = case.n - int(fm.sum()) + int(case.U.sum())
    assert abs(h["mu"] * pairs - h["gap"]) <= 1e-14 * h["gap"] and pairs < case.n + int(case.U.sum())
    _assert_all(cell, e, {k: _bound_free(k) for k in e})


CELLS = [("1x2", False, None), ("40x600", False, None), ("40x600b", False, None), ("40x600b-interleaved", False, None),
         ("5x50-all-but-one", False, None), ("sparse/130x300", True, "dense"), ("sparse/130x300", True, "sparse"),
         ("sparse/130x300b", True, "dense"), ("sparse/130x300b", True, "sparse"), ("sparse/8x16500", True, None)]
CELL_IDS = ["%s%s" % (c[0], "-" + c[2] if c[2] else "") for c in CELLS]


def _cell_solver(name, as_sparse, factor, rho=RHO, **kw):
    case, free = FL.get(name)
    A = sparse.csc_matrix(case.A) if as_sparse else case.A
    if factor is not None:
        kw["factor"] = factor
    return ipm.IpmSolver(A, case.b, case.c, ub=case.ub(), free_lp=free, free_rho=rho, **kw)


@pytest.mark.parametrize("name,as_sparse,factor", CELLS, ids=CELL_IDS)
def test_one_iteration(name, as_sparse, factor):
    case, free = FL.get(name)
    with _cell_solver(name, as_sparse, factor) as sv:
        sch = sv.schedule()
        assert sch["fused_small"] == 0 and sv.sparse == as_sparse and sv.bounded == int(case.U.sum())
        if factor == "sparse":
            assert sv.factor == "sparse" and sv.factor_info()["panels"] >= 1
        elif factor == "dense":
            assert sv.factor == "dense" and sch["blocks"] == (case.m + 127) // 128
        check_free_lp_iteration("%s/factor=%s" % (name, factor), sv, case, free, FL.oracle(name))


def test_default_rho_reaches_the_scaling_exactly():
    case, free = FL.get("40x600b")
    with _cell_solver("40x600b", False, None, rho=None) as sv:
        assert sv.free_lp_columns()[1] == 1e-8
        sv.set_state(*case.state())
        sv.newton_direction(False)
        d = sv.debug_column_vector("d")
        assert np.all(d[free] == 1.0 / 1e-8) and np.all(np.delete(d, free) < 1e3)


# ---- 2. iteration sequences and the start -------------------------------------------------------------------------------------
def _bits(sv):
    out = [v.tobytes() for v in sv.get_state()]
    wz = sv.get_bound_state()
    return out + ([] if wz is None else [v.tobytes() for v in wz])


def _record_bytes(records):
    """Statistics or history records as bytes: bit for bit, and a NaN equals itself."""
    return np.array([[float(r[k]) for k in sorted(r) if k not in ("solve_ms", "k", "iterations")] for r in records]).tobytes()


@pytest.mark.parametrize("name,as_sparse,factor", [("40x600b", False, None), ("sparse/130x300b", True, "sparse")], ids=["dense", "sparse-factor"])
def test_three_steps_at_once_equal_three_single_steps(name, as_sparse, factor):
    case, free = FL.get(name)
    out = []
    for steps in ((3,), (1, 1, 1)):
        with _cell_solver(name, as_sparse, factor) as sv:
            sv.set_state(*case.state())
            for k in steps:
                st = sv.iterate(k)
            out.append((_bits(sv), _record_bytes([st])))
            assert np.all(np.isfinite(sv.get_state()[0]))
    assert out[0] == out[1]


def _rel(a, ref):
    return float(np.max(np.abs(np.ravel(a) - np.ravel(ref))) / max(1e-300, float(np.max(np.abs(ref)))))


def _device_state(sv):
    x, y, s = (v.ravel() for v in sv.get_state())
    wz = sv.get_bound_state()
    w, z = (v.ravel() for v in wz) if wz is not None else (np.zeros(sv.n), np.zeros(sv.n))
    return x, y, s, w, z


@pytest.mark.parametrize("name,as_sparse,kw", [("8x20", False, {}), ("40x130b", False, {}), ("200x520", True, {"factor": "sparse"})],
                         ids=["plain", "bounded", "sparse-factor"])
def test_device_start_matches_the_restated_host_start(name, as_sparse, kw):
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    ref = FL.mehrotra_start64(A, b, c, u, free)
    with ipm.IpmSolver(sparse.csc_matrix(A) if as_sparse else A, b, c, ub=u, free_lp=free, **kw) as sv:
        host = [np.asarray(v, dtype=np.float64).ravel() for v in sv.mehrotra_start()]
        host = tuple(host) if len(host) == 5 else tuple(host) + (np.zeros(sv.n), np.zeros(sv.n))
        assert sv.init_state_mehrotra() == 0
        dev = _device_state(sv)
        names = ("x", "y", "s") + (("w", "z") if u is not None else ())
        e_host = max(_rel(h, r) for h, r, _ in zip(host, ref, names))
        e_dev = {k: _rel(d, r) for d, r, k in zip(dev, ref, names)}
        tol = max(10.0 * e_host, 1e-13)
        print("OBS start %s host %.3e device %s allowed %.3e" % (name, e_host, " ".join("%s=%.2e" % kv for kv in e_dev.items()), tol))
        assert max(e_dev.values()) <= tol, (e_dev, e_host, tol)
        x, y, s, w, z = dev
        assert np.all(s[free] == 0) and np.all(w[free] == 0) and np.all(z[free] == 0)
        assert np.delete(x, free).min() > 0 and np.delete(s, free).min() > 0
        st = sv.solve(tol=TOL)                                   # and the solve from it converges like the host loop from its own
        assert st["status"] == 1 and abs(st["iterations"] - FL.host_loop(name, "mehrotra")["iterations"]) <= 2


@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_device_start_degenerate_fallback(bounded):
    """b = 0 and c = 0: x = 0 and s = 0 from least squares, every barrier sum is 0 -> the reference's start of such a handle, exactly."""
    A = np.random.default_rng(5).standard_normal((6, 20))
    u = None
    if bounded:
        u = np.full(20, np.inf)
        u[[2, 9]] = 3.0
    free = np.array([4, 11], dtype=np.int32)
    with ipm.IpmSolver(A, np.zeros(6), np.zeros(20), ub=u, free_lp=free, dense=True) as sv:
        sv.init_state_mehrotra()
        x, y, s, w, z = _device_state(sv)
        host = sv.mehrotra_start()
    want_s = np.ones(20)
    want_s[free] = 0.0
    assert np.all(x == 1) and np.all(y == 1) and np.array_equal(s, want_s)
    assert np.array_equal(host[0], x) and np.array_equal(host[2], s)
    if bounded:
        U = np.isfinite(u)
        assert np.all(w[U] == 1) and np.all(z[U] == 1) and not w[~U].any() and not z[~U].any()


# ---- 3. whole solves ----------------------------------------------------------------------------------------------------------
SOLVES = [("1x2", False, {}), ("40x130b", False, {}), ("200x520", True, {"factor": "dense"}), ("200x520", True, {"factor": "sparse"}),
          ("40x130dep", False, {})]
SOLVE_IDS = ["%s%s" % (c[0], "-" + c[2]["factor"] if c[2] else "") for c in SOLVES]


def check_solve(cell, name, x, y, s, info, dependent=False):
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    ref = FL.host_loop(name)
    x, y, s = x.ravel(), y.ravel(), s.ravel()
    assert info["status"] == 1, (cell, info["status"], info["iterations"])
    assert info["free_lp"] == free.shape[0] and info["free"] == 0 and info["quadratic"] == 0
    w = info["w"].ravel() if u is not None else None
    z = info["z"].ravel() if u is not None else None
    rp, rd, gap = Q.stop_test_ld(A, b, c, np.zeros(A.shape[1]), u, x, y, s, w, z)
    x_err = float(np.linalg.norm(x - xs) / np.linalg.norm(xs))
    obj_err = abs(info["objective"] - ref["obj_star"]) / abs(ref["obj_star"])
    host_obj_err = abs(ref["objective"] - ref["obj_star"]) / abs(ref["obj_star"])
    print("OBS %s iterations %d (host %d) rp %.3e rd %.3e gap %.3e x_err %.3e (host %.3e) obj_err %.3e (host %.3e) fixed %d alpha_p %.3f alpha_d %.3f"
          % (cell, info["iterations"], ref["iterations"], rp, rd, gap, x_err, ref["x_err"], obj_err, host_obj_err, info["pivots_fixed"],
             info["alpha_p"], info["alpha_d"]))
    assert abs(info["iterations"] - ref["iterations"]) <= 2, (cell, info["iterations"], ref["iterations"])
    assert rp <= 2 * TOL and rd <= 2 * TOL and gap <= 2 * TOL, (cell, rp, rd, gap)
    if not dependent:
        assert x_err <= max(1e-9, 100 * ref["x_err"]), (cell, x_err, ref["x_err"])
    assert obj_err <= max(1e-9, 100 * host_obj_err), (cell, obj_err, host_obj_err)
    assert np.all(s[free] == 0) and np.all(np.delete(s, free) >= 0) and np.all(np.delete(x, free) > 0)


@pytest.mark.parametrize("name,as_sparse,kw", SOLVES, ids=SOLVE_IDS)
def test_whole_solve(name, as_sparse, kw):
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    x, y, s, info = ipm.solve_with_info(sparse.csc_matrix(A) if as_sparse else A, b, c, ub=u, free_lp=free, tol=TOL, **kw)
    assert x.shape == (A.shape[1], 1) and y.shape == (A.shape[0], 1) and s.shape == x.shape
    if kw:
        assert info["factor_path"] == kw["factor"]
    check_solve("%s/%s" % (name, kw.get("factor", "dense-ingest")), name, x, y, s, info, dependent=name.endswith("dep"))
    if not name.endswith("dep"):
        assert (x.ravel()[free] < 0).any() or free.shape[0] == 1          # free columns of either sign


def test_the_fused_launch_with_the_residual_stream():
    """The smallest dense shape with both: the fused formation + factorization and the residual stream exist from 16 blocks of 128
    rows on (host_fused.h: ff_min_nblk; ipm_create: stream3), i.e. m = 15 x 128 + 1."""
    name = "1921x4096"
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    with ipm.IpmSolver(A, b, c, free_lp=free) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=TOL)
        sch = sv.schedule()
        assert sch["fused_factor"] == 1 and sch["fused_small"] == 0 and sch["blocks"] == 16 and sch["stream_at"] == 1, sch
        x, y, s = sv.get_state()
        info = dict(st, free_lp=sv._n_free_lp, free=0, quadratic=0)
        check_solve(name, name, x, y, s, info)


# ---- 4. invariants ----------------------------------------------------------------------------------------------------------
def _run(name, free_lp="problem", after=None, max_iter=5000, as_sparse=False, rho=None, **kw):
    """A fresh handle on that problem -> (statistics, (records, their bytes), the state's bytes).
    free_lp: the constructor's ("problem": the problem's own); after(sv): called before the start."""
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    with ipm.IpmSolver(sparse.csc_matrix(A) if as_sparse else A, b, c, ub=u, free_lp=free if isinstance(free_lp, str) else free_lp, free_rho=rho, **kw) as sv:
        if after:
            after(sv)
        sv.init_state(1.0)
        st = sv.solve(tol=TOL, max_iter=max_iter)
        hist = sv.history()
        return st, (len(hist), _record_bytes([st]), _record_bytes(hist)), _bits(sv)


NAME = "40x130b"          # bounded, dense ingest; 8x20 for the plain kernels


@pytest.mark.parametrize("name", [NAME, "8x20"])
def test_bitwise_repeat(name):
    a, b = _run(name), _run(name)
    assert a[0]["status"] == 1 and a[1:] == b[1:]


@pytest.mark.parametrize("name", [NAME, "8x20"])
def test_set_then_cleared_equals_never_set(name):
    never = _run(name, free_lp=None, max_iter=6)
    assert never[1][0] > 0
    for how in (lambda sv: sv.set_free_lp(None), lambda sv: sv.set_free_lp([]), lambda sv: sv._check(sv._lib.ipm_set_free_lp_columns(sv._h, None, 3, 0.0))):
        def clear(sv, how=how):
            assert sv.free_lp_columns()[0].shape[0] > 0
            how(sv)
            assert sv.free_lp_columns()[0].shape[0] == 0
        assert _run(name, after=clear, max_iter=6)[1:] == never[1:]
    assert _run(name, max_iter=6)[1] != never[1]                               # (and the set does change the trajectory)


@pytest.mark.parametrize("name", [NAME, "8x20"])
def test_order_of_the_setters(name):
    """The constructor sets the free set, then A, then the bounds.  The set after all of them gives the same solve bit for bit."""
    free = FL.problem(name)[3]
    ctor = _run(name)

    def after_A(sv):
        assert sv.free_lp_columns()[0].shape[0] == 0
        sv.set_free_lp(free)
    assert _run(name, free_lp=None, after=after_A)[1:] == ctor[1:]
    assert ctor[0]["status"] == 1


def test_independent_of_check_every():
    a, b = _run(NAME, check_every=1), _run(NAME, check_every=7)
    assert a[0]["status"] == 1 and a[1:] == b[1:]


@pytest.mark.parametrize("name,as_sparse,kw", [(NAME, False, {}), ("200x520", True, {"factor": "sparse"})], ids=["dense", "sparse-factor"])
def test_independent_of_what_device_memory_held(name, as_sparse, kw, monkeypatch):
    """The rule of tests/test_gpu_residue.py for the handle's new allocation (the byte marks): with every allocation of the library
    filled with 0x00 or 0xFF bytes before its first use, the solve is the one of an unfilled handle, bit for bit."""
    plain = _run(name, as_sparse=as_sparse, **kw)
    assert plain[0]["status"] == 1
    for fill in ("0", "255"):
        monkeypatch.setenv("IPM_TEST_ALLOC_FILL", fill)
        assert _run(name, as_sparse=as_sparse, **kw)[1:] == plain[1:], fill


@pytest.mark.parametrize("name", [NAME, "8x20"])
def test_equilibration_equals_the_prescaled_problem(name):
    """The rule of tests/test_gpu_equilibrate.py: scale="ruiz" is bit-identical, after unscaling, to an unscaled handle given the
    host-prescaled (R A C, R b, C c, u / C) with the same free set and the same rho: rho applies in the handle's units."""
    A_, b_, c_, free, u_, xs, ys, ss = FL.problem(name)
    rng = np.random.default_rng(11)
    dr, dc = 10.0 ** rng.uniform(-3, 3, A_.shape[0]), 10.0 ** rng.uniform(-3, 3, A_.shape[1])
    A, b, c, u = dr[:, None] * A_ * dc[None, :], dr * b_, dc * c_, (None if u_ is None else u_ / dc)
    er, ec, changed = EO.ruiz(A, 16)
    assert 0 < changed < 16
    R, Cc = EO.factors(er, ec)
    A2, b2, c2, u2 = EO.prescale(A, b, c, u, er, ec)
    out = []
    for scaled in (True, False):
        args, ub = ((A, b, c), u) if scaled else ((A2, b2, c2), u2)
        with ipm.IpmSolver(*args, ub=ub, scale="ruiz" if scaled else None, free_lp=free, free_rho=1e-6) as sv:
            if scaled:
                assert np.array_equal(sv.scaling()[1], Cc) and sv.scale_info["passes"] == changed
            assert np.array_equal(sv.free_lp_columns()[0], free) and sv.free_lp_columns()[1] == 1e-6
            sv.init_state(1.0)
            st = sv.solve(tol=TOL, max_iter=40)
            out.append((st, sv.history(), sv.get_state(), sv.get_bound_state()))
    (st1, h1, (x1, y1, s1), wz1), (st2, h2, (x2, y2, s2), wz2) = out
    for k in ("status", "iterations", "objective", "rp_norm", "rd_norm", "gap", "b_norm", "c_norm", "alpha_p", "alpha_d"):
        assert st1[k] == st2[k], (k, st1[k], st2[k])
    assert st1["iterations"] > 0 and _record_bytes(h1) == _record_bytes(h2)
    Rc, Cv = R.reshape(-1, 1), Cc.reshape(-1, 1)
    assert np.array_equal(x1, Cv * x2) and np.array_equal(y1, Rc * y2) and np.array_equal(s1, s2 / Cv)
    assert np.all(s1.ravel()[free] == 0)
    if u is not None:
        assert np.array_equal(wz1[0], Cv * wz2[0]) and np.array_equal(wz1[1], wz2[1] / Cv)


def test_refined_solve_agrees():
    A, b, c, free, u, xs, ys, ss = FL.problem("200x520")
    plain = ipm.solve_with_info(A, b, c, free_lp=free, tol=TOL)[3]
    refined = ipm.solve_with_info(A, b, c, free_lp=free, tol=TOL, refine=2)[3]
    assert plain["status"] == 1 and refined["status"] == 1 and refined["refine"].k == 2 and refined["refine"].solves > 0
    assert abs(refined["objective"] - plain["objective"]) <= 1e-8 * abs(plain["objective"])


def test_dense_column_split_solve_agrees():
    """The dense-column split of the sparse factor serves a handle with LP free columns: it reads only d.  The linking columns are
    the free ones (c adjusted so the problem stays dual feasible: c_j = (A^T y0)_j there is what s_j = 0 needs)."""
    A, b, c, cols = workloads.block_angular_lp(400, 50, 8, seed=1)
    b, c = b.ravel(), c.ravel().copy()
    out = []
    for kw in ({}, {"dense_cols": cols}):
        x, y, s, info = ipm.solve_with_info(A, b, c, free_lp=cols, factor="sparse", tol=TOL, **kw)
        print("OBS split %s status %d iterations %d objective %.12e fixed %d" % (sorted(kw), info["status"], info["iterations"], info["objective"], info["pivots_fixed"]))
        assert info["status"] == 1 and info["factor_path"] == "sparse" and info["free_lp"] == 8
        out.append(info)
    unsplit, split = out
    assert unsplit["dense_cols"] is None and split["dense_cols"]["k"] == 8 and split["dense_cols"]["corrections"] > 0
    assert abs(split["objective"] - unsplit["objective"]) <= 1e-8 * abs(unsplit["objective"])


# ---- 5. state seams and refusals ----------------------------------------------------------------------------------------------
def _handle(name=NAME, free_lp="problem", **kw):
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    return ipm.IpmSolver(A, b, c, ub=kw.pop("ub", u), free_lp=free if isinstance(free_lp, str) else free_lp, **kw), free


def test_state_seams():
    sv, fr = _handle()
    with sv:
        sv.init_state(1.0)
        x, y, s = (v.ravel() for v in sv.get_state())
        assert np.all(s[fr] == 0) and np.all(x == 1) and np.all(np.delete(s, fr) == 1)
        sv.set_state(np.full(sv.n, 2.0), np.zeros(sv.m), np.full(sv.n, 3.0))
        x, y, s = (v.ravel() for v in sv.get_state())
        assert np.all(s[fr] == 0) and np.all(np.delete(s, fr) == 3) and np.all(x == 2)
        sv.set_free_lp(fr[:2])                                                  # changed on a handle that holds a state
        assert np.array_equal(sv.free_lp_columns()[0], fr[:2]) and np.all(sv.get_state()[2].ravel()[fr] == 0)
        sv.set_state(np.full(sv.n, 2.0), np.zeros(sv.m), np.full(sv.n, 3.0))
        sv.set_free_lp(fr[1:4], 1e-6)                                           # s goes to 0 on the NEW free columns; elsewhere it stays what was stored
        s = sv.get_state()[2].ravel()
        assert np.all(s[fr[1:4]] == 0) and s[fr[0]] == 0 and s[fr[4]] == 3 and sv.free_lp_columns()[1] == 1e-6
        sv.set_free_lp(None)                                                    # cleared: the former free columns still hold s = 0 ...
        assert sv.free_lp_columns()[0].shape[0] == 0 and np.all(sv.get_state()[2].ravel()[fr[1:4]] == 0)
        sv.init_state(1.0)                                                      # ... so the caller sets a state anew, as the header says
        assert np.all(sv.get_state()[2] == 1)
        st = sv.iterate(2)
        assert st["iterations"] == 2 and np.all(np.isfinite(sv.get_state()[0])) and np.all(sv.get_state()[2] > 0)


def _refused(sv, code, word, call):
    rc = call()
    assert rc == code, (rc, sv._lib.ipm_last_error(sv._h))
    assert word.encode() in sv._lib.ipm_last_error(sv._h), sv._lib.ipm_last_error(sv._h)


def test_bad_arguments_are_refused_and_the_set_is_kept():
    sv, fr = _handle()
    with sv:
        lib, h = sv._lib, sv._h
        for idx, word in (([int(fr[0]), sv.n], "out of range"), ([-1], "out of range"), ([int(fr[0]), int(fr[1]), int(fr[0])], "duplicated")):
            a = np.array(idx, dtype=np.int32)
            _refused(sv, -1, word, lambda: lib.ipm_set_free_lp_columns(h, _iptr(a), len(idx), 0.0))
            assert np.array_equal(sv.free_lp_columns()[0], fr)
        _refused(sv, -1, "count", lambda: lib.ipm_set_free_lp_columns(h, _iptr(fr), -2, 0.0))
        for bad in (np.inf, -np.inf, np.nan):
            _refused(sv, -1, "not finite", lambda: lib.ipm_set_free_lp_columns(h, _iptr(fr), fr.shape[0], bad))
        assert sv.free_lp_columns()[1] == 1e-8
        assert lib.ipm_set_free_lp_columns(h, _iptr(fr), fr.shape[0], -3.0) == 0 and sv.free_lp_columns()[1] == 1e-8      # rho <= 0: the default
        k, rho = C.c_int32(0), C.c_double(0)
        two = np.zeros(2, dtype=np.int32)
        assert lib.ipm_get_free_lp_columns(h, _iptr(two), 2, C.byref(k), C.byref(rho)) == 0 and k.value == fr.shape[0] and np.array_equal(two, fr[:2])
        with pytest.raises(ValueError, match="out of range"):
            sv.set_free_lp([sv.n])
        with pytest.raises(ValueError, match="twice"):
            sv.set_free_lp([1, 1])
        with pytest.raises(ValueError, match="not finite"):
            sv.set_free_lp([1], np.inf)


def test_finite_bound_in_both_orders():
    A, b, c, fr, u_, xs, ys, ss = FL.problem(NAME)
    ub = u_.copy()
    ub[fr[2]] = 5.0
    sv, _ = _handle()
    with sv:                                                                    # the set first
        _refused(sv, -1, "LP free column", lambda: sv._lib.ipm_set_bounds(sv._h, _dptr(ub)))
        assert sv.bounded == int(np.isfinite(u_).sum()) and np.array_equal(sv.free_lp_columns()[0], fr)
        sv.init_state(1.0)
        assert sv.solve(tol=TOL)["status"] == 1                                 # the handle kept its bounds and stays usable
    sv, _ = _handle(free_lp=None, ub=ub)
    with sv:                                                                    # the bound first
        with pytest.raises(ipm.IpmError, match="finite upper bound") as ei:
            sv.set_free_lp(fr)
        assert ei.value.code == -1 and sv.free_lp_columns()[0].shape[0] == 0
        sv.set_free_lp(np.delete(fr, 2))


def test_no_pair_left_is_refused():
    A, b, c, fr, u, xs, ys, ss = FL.problem("8x20")
    with ipm.IpmSolver(A, b, c, dense=True) as sv:
        every = np.arange(sv.n, dtype=np.int32)
        _refused(sv, -1, "no complementarity pair", lambda: sv._lib.ipm_set_free_lp_columns(sv._h, _iptr(every), sv.n, 0.0))
        sv.set_free_lp(every[1:])                                               # one pair is enough (test_one_iteration: all but one)


def test_quadratic_and_curvature_sets_in_both_orders():
    A, b, c, fr, u, xs, ys, ss = FL.problem("8x20")
    g = np.full(20, 0.5)
    with ipm.IpmSolver(A, b, c, dense=True, free_lp=fr) as sv:                  # the LP free set first
        with pytest.raises(ipm.IpmError, match="LP free columns") as ei:
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
        with pytest.raises(ipm.IpmError, match="LP free columns") as ei:
            sv.set_free([0])
        assert ei.value.code == -1 and sv.free_columns().shape[0] == 0 and np.array_equal(sv.free_lp_columns()[0], fr)
        sv.set_quadratic(None)                                                  # clearing is always accepted
        sv.set_free(None)
    with ipm.IpmSolver(A, b, c, dense=True, quad=g) as sv:                      # the term first
        with pytest.raises(ipm.IpmError, match="quadratic term") as ei:
            sv.set_free_lp(fr)
        assert ei.value.code == -1 and sv.free_lp_columns()[0].shape[0] == 0
    with ipm.IpmSolver(A, b, c, dense=True, quad=g, free=[0]) as sv:            # the curvature set first (g cleared: the set remains)
        with pytest.raises(ipm.IpmError, match="quadratic term"):
            sv.set_free_lp(fr)
    with ipm.IpmSolver(A, b, c, dense=True) as sv:
        sv.set_free([0])                                                        # (accepted on an LP handle; refused later without a term)
        with pytest.raises(ipm.IpmError, match="ipm_set_free_columns") as ei:
            sv.set_free_lp(fr)
        assert ei.value.code == -1


def test_lockstep_detect_and_corrector_handles_refuse():
    A, b, c, fr, u, xs, ys, ss = FL.problem("200x520")
    with ipm.IpmSolver(sparse.csc_matrix(A), b, c, lockstep=True, factor="dense") as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_LOCKSTEP") as ei:
            sv.set_free_lp(fr)
        assert ei.value.code == -1 and sv.free_lp_columns()[0].shape[0] == 0
        sv.set_free_lp(None)                                                    # clearing is always accepted
    with ipm.IpmSolver(A, b, c, detect_infeasibility=True) as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_DETECT_INFEASIBILITY") as ei:
            sv.set_free_lp(fr)
        assert ei.value.code == -1
    with ipm.IpmSolver(A, b, c, correctors=2) as sv:                            # correctors first
        with pytest.raises(ipm.IpmError, match="centrality correctors") as ei:
            sv.set_free_lp(fr)
        assert ei.value.code == -1
        sv.set_correctors(0)
        sv.set_free_lp(fr)
    with ipm.IpmSolver(A, b, c, free_lp=fr) as sv:                              # the set first
        with pytest.raises(ipm.IpmError, match="LP free columns") as ei:
            sv.set_correctors(1)
        assert ei.value.code == -1 and sv.correctors == 0
        sv.set_correctors(0)


def test_small_path_in_both_orders():
    A, b, c, fr, u, xs, ys, ss = FL.problem("40x130b")
    A = sparse.csc_matrix(A)
    with ipm.IpmSolver(A, b, c, ub=u) as sv:                                    # A first: the one-workgroup path is taken ...
        assert sv.schedule()["fused_small"] == 1
        with pytest.raises(ipm.IpmError, match="before A") as ei:               # ... and a free set then is refused
            sv.set_free_lp(fr)
        assert ei.value.code == -1 and sv.free_lp_columns()[0].shape[0] == 0
        sv.set_free_lp(None)
        sv.init_state(1.0)
        assert sv.solve(tol=TOL, max_iter=3)["iterations"] > 0                  # and the handle stays usable
    with ipm.IpmSolver(A, b, c, ub=u, free_lp=fr) as sv:                        # the set first: the multi-kernel path
        assert sv.schedule()["fused_small"] == 0 and np.array_equal(sv.free_lp_columns()[0], fr)
        sv.init_state(1.0)
        assert sv.solve(tol=TOL)["status"] == 1


def test_mehrotra_start_keeps_its_refusal_for_the_curvature_set():
    A, b, c, fr, u, xs, ys, ss = FL.problem("8x20")
    with ipm.IpmSolver(A, b, c, dense=True, quad=np.full(20, 0.5), free=[0]) as sv:
        with pytest.raises(ipm.IpmError, match="ipm_init_state_mehrotra") as ei:
            sv.init_state_mehrotra()
        assert ei.value.code == -1


def test_general_form_front_end():
    """A small constructed general-form LP with inequality rows, a shifted lower bound, a free variable and a (-inf, ub] variable,
    against its constructed optimum (the variables in the native form's own coordinates come from workloads.free_lp)."""
    from test_free_lp_host import general_form_problem
    P = general_form_problem()
    obj, info = general_form.new_interior_sparse(P["c"], Aeq=P["Aeq"], beq=P["beq"], Aineq=P["Aineq"], bineq=P["bineq"], lb=P["lb"], ub=P["ub"],
                                                 tol=1e-9, bounds="native", free="native", return_info=True)
    x_err = float(np.linalg.norm(info["x"] - P["x_star"]) / np.linalg.norm(P["x_star"]))
    print("OBS general status %d iterations %d obj_err %.3e x_err %.3e" % (info["status"], info["iterations"], abs(obj - P["obj_star"]), x_err))
    assert info["status"] == 1 and info["free_lp"] == P["n_free"] and info["bounded"] == P["n_bounded"]
    assert abs(obj - P["obj_star"]) <= 1e-6 * max(1.0, abs(P["obj_star"])) and x_err <= 1e-6
    with pytest.raises(ValueError, match="bounds=\"native\""):
        general_form.new_interior_sparse(P["c"], Aeq=P["Aeq"], beq=P["beq"], lb=P["lb"], ub=P["ub"], bounds="fold", free="native")
