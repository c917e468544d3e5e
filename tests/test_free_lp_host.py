"""LP free columns, host side: the restatement of the rule (tests/free_lp_oracle.py), the policy on constructed optima,
the general-form front end, every ValueError, the ABI bindings and the variant tables with the fifth class switch.  No GPU.

Bounds.  The float64 restatement against its own longdouble run: 1e-12 at free_lp_oracle.ITER_RHO (which says why the one-iteration
comparisons do not run at the default rho = 1e-8: cond(A Theta A^T) eps = 1e-8 there, for any float64 code).  The unreduced Newton
system in longdouble: 1e-15 relative to the largest term of each row block (the elimination is exact algebra; longdouble rounds at
5e-20 and the normal matrix of these interior states has a condition number below 1e4).  The constructed optima: the stop test ran
at tol = 1e-8 with strictly complementary optima whose nonzero x*, s* lie in [0.5, 2], so ||x - x*|| / ||x*|| <= 1e-6 leaves two
orders for the conditioning of the basis (observed: 8e-11 .. 5e-9), and the objective agrees to 1e-7 relative.
"""
import ctypes as C
import inspect

import numpy as np
import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batch, batches, general_form, handle, workloads

import free_lp_oracle as FL
import iteration_oracle as IO

LD = IO.LD
HOST_CELLS = ["1x2", "40x600", "40x600b", "40x600b-interleaved", "5x50-all-but-one", "sparse/130x300b"]
KEYS = ("rc", "theta", "va", "qa", "dxa", "dya", "dsa", "dwa", "dza", "v", "q", "dx", "dy", "ds", "dw", "dz", "xn", "yn", "sn", "wn", "zn")
SCALARS = ("alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "mu", "mu_aff", "sigma", "gap", "objective")


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOST_CELLS)
def test_float64_agrees_with_longdouble_on_one_iteration(name):
    case, free = FL.get(name)
    o, h = FL.oracle(name), FL.iterate(case, free, T=np.float64)
    errs = {k: IO.rel(h[k], o[k]) for k in KEYS}
    errs.update({k: float(abs(LD(h[k]) - o[k]) / abs(o[k])) for k in SCALARS})
    bad = {k: v for k, v in errs.items() if not v <= 1e-12}
    assert not bad, (name, bad)
    fm = FL.free_mask(free, case.n)
    assert np.all(h["sn"][fm] == 0) and np.all(h["ds"][fm] == 0) and np.all(h["q"][fm] == 0) and np.all(h["theta"][fm] == 1.0 / FL.ITER_RHO)


def test_float64_at_the_default_rho_is_bounded_by_the_conditioning():
    """Recorded, not a defect: at rho = 1e-8 the two precisions agree to cond eps ~ 1e-8 only (free_lp_oracle.ITER_RHO)."""
    case, free = FL.get("40x600b")
    o, h = FL.iterate(case, free, FL.RHO), FL.iterate(case, free, FL.RHO, T=np.float64)
    worst = max(IO.rel(h[k], o[k]) for k in ("dx", "dy", "ds", "xn", "yn", "sn"))
    assert 1e-12 < worst <= 1e-6, worst


@pytest.mark.parametrize("bounded", [False, True])
def test_empty_set_reproduces_the_lp_oracle_bit_for_bit(bounded):
    case = IO.interior_case(40, 130, bounded, 2)
    a, b = IO.iterate(case), FL.iterate(case, None)
    for k in ("dxa", "dya", "dsa", "dwa", "dza", "atdya", "dx", "dy", "ds", "dw", "dz", "atdy", "xn", "yn", "sn", "wn", "zn", "atyn",
              "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "mu", "mu_aff", "sigma", "gap", "objective", "rp_norm", "rd_norm"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", HOST_CELLS)
def test_directions_satisfy_the_unreduced_newton_system(name):
    """Without the elimination: A dx = -r_b; barrier rows A^T dy + ds - dz = -r_c, s dx + x ds = -r_3; FREE rows A^T dy - rho dx = -r_c,
    ds = 0; on U dx + dw = -r_u, z dw + w dz = -r_4.  Both directions, in longdouble."""
    case, free = FL.get(name)
    o = FL.oracle(name)
    fm = FL.free_mask(free, case.n)
    nf, U = ~fm, case.U
    A = case.A.astype(LD)
    x, s, w, z = (np.asarray(v, dtype=LD) for v in (case.x, case.s, case.w, case.z))
    s = np.where(fm, LD(0), s)
    rho = LD(FL.ITER_RHO)
    for tag, r3, r4 in (("a", x * s, w * z), ("", o["r3c"], o["r4c"])):
        dx, dy, ds, dw, dz = (o[k + tag] for k in ("dx", "dy", "ds", "dw", "dz"))
        atdy = A.T @ dy

        def small(res, *terms):
            return float(IO.norm(res)) <= 1e-15 * max(float(IO.norm(t)) for t in terms)
        assert small(A @ dx + o["rb"], A @ dx, o["rb"])
        assert small((atdy + ds - dz + o["rc"])[nf], atdy[nf], o["rc"][nf])
        assert small((s * dx + x * ds + r3)[nf], (s * dx)[nf], (x * ds)[nf])
        assert small((atdy - rho * dx + o["rc"])[fm], atdy[fm], o["rc"][fm]) and np.all(ds[fm] == 0)
        if U.any():
            assert small((dx + dw + o["ru"])[U], dx[U], dw[U])
            assert small((z * dw + w * dz + r4)[U], (z * dw)[U], (w * dz)[U])
        assert np.all(dw[~U] == 0) and np.all(dz[~U] == 0)


# ---- the policy on constructed optima -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["reference", "mehrotra"])
@pytest.mark.parametrize("name", ["1x2", "8x20", "40x130b", "200x520", "40x130dep"])
def test_host_loop_reaches_the_constructed_optimum(name, start):
    A, b, c, free, u, xs, ys, ss = FL.problem(name)
    r = FL.host_loop(name, start)
    assert r["converged"] and r["iterations"] <= 20, (name, r["iterations"])
    assert abs(r["objective"] - r["obj_star"]) <= 1e-7 * max(1.0, abs(r["obj_star"]))
    assert np.linalg.norm(A @ r["x"] - b) <= 1e-8 * (1 + np.linalg.norm(b))
    assert np.all(r["s"][free] == 0)
    if not name.endswith("dep"):
        assert r["x_err"] <= 1e-6 and r["y_err"] <= 1e-6, (name, r["x_err"], r["y_err"])
        assert (r["x"][free] < 0).any() or free.shape[0] == 1


def test_host_loop_iteration_count_does_not_depend_on_rho():
    counts = {rho: FL.host_loop("40x130b", "reference", rho)["iterations"] for rho in (1e-4, 1e-6, 1e-8, 1e-10)}
    assert max(counts.values()) - min(counts.values()) <= 1, counts


def test_workload_free_lp():
    A, b, c, free, u, xs, ys, ss = workloads.free_lp(40, 130, 10, 7, bounded=True)
    n = 130
    fm = FL.free_mask(free, n)
    U = np.isfinite(u)
    z = A.T @ ys + ss - c                                         # c = A^T y + s - z
    assert free.dtype == np.int32 and free.shape == (10,) and np.all(np.diff(free) > 0) and not (fm & U).any()
    assert np.array_equal(A @ xs, b) and np.all(ss[fm] == 0) and (xs[free] < 0).any() and (xs[free] > 0).any()
    assert np.all(xs[~fm] >= 0) and np.all(ss >= 0) and np.all(xs[~fm] * ss[~fm] == 0) and np.all(xs[U] <= u[U]) and np.all(z >= -1e-15)
    at = U & (xs == u)
    assert at.any() and np.all(z[at] >= 0.5 - 1e-12) and np.all(np.abs(z[~at]) <= 1e-14)
    basic = ~fm & (xs > 0) & ~at
    assert int(basic.sum()) == 40 - 10 and np.all((xs[~fm] > 0) | (ss[~fm] > 0))          # strictly complementary, m - n_free basic
    A2, b2, c2, f2, u2, x2, y2, s2 = workloads.free_lp(40, 130, 10, 7, dependent=True)
    assert u2 is None and np.array_equal(A2[:, f2[-1]], A2[:, f2[0]]) and np.array_equal(A2[:, f2[-2]], 2.0 * A2[:, f2[1]])
    assert c2[f2[-1]] == c2[f2[0]] and abs(c2[f2[-2]] - 2.0 * c2[f2[1]]) <= 1e-14
    same = workloads.free_lp(40, 130, 10, 7, bounded=True)
    assert all(np.array_equal(p, q) for p, q in zip((A, b, c, free, u, xs, ys, ss), same))
    for bad in (dict(m=4, n=10, n_free=0), dict(m=4, n=10, n_free=10), dict(m=4, n=10, n_free=6)):
        with pytest.raises(ValueError):
            workloads.free_lp(seed=0, **bad)
    with pytest.raises(ValueError, match="n_free >= 4"):
        workloads.free_lp(8, 20, 3, 0, dependent=True)


def test_restated_mehrotra_start_rules():
    A, b, c, free, u, xs, ys, ss = FL.problem("40x130b")
    x, y, s, w, z = FL.mehrotra_start64(A, b, c, u, free)
    U = np.isfinite(u)
    ls = A.T @ np.linalg.solve(A @ A.T, b)
    assert np.array_equal(x[free], ls[free]) and np.all(s[free] == 0) and np.all(w[free] == 0) and np.all(z[free] == 0)
    assert np.delete(x, free).min() > 0 and np.delete(s, free).min() > 0 and w[U].min() > 0 and z[U].min() > 0
    x0, y0, s0, w0, z0 = FL.mehrotra_start64(A, np.zeros_like(b), np.zeros_like(c), u, free)          # degenerate: the reference's start
    assert np.all(x0 == 1) and np.all(y0 == 1) and np.all(s0[free] == 0) and np.all(np.delete(s0, free) == 1) and np.array_equal(w0, U * 1.0)


# ---- the general-form front end -----------------------------------------------------------------------------------------------
def test_native_form_entry_for_entry():
    """Three variables: x0 free, x1 in (-inf, 4], x2 in [1.5, 6]; one inequality row, one equality row."""
    c = [2.0, -3.0, 5.0]
    Aineq, bineq = np.array([[1.0, 2.0, -1.0]]), [7.0]
    Aeq, beq = np.array([[3.0, -1.0, 4.0]]), [9.0]
    lb, ub = [-np.inf, -np.inf, 1.5], [np.inf, 4.0, 6.0]
    F = general_form.native_form(c, Aeq=Aeq, beq=beq, Aineq=Aineq, bineq=bineq, lb=lb, ub=ub, free="native")
    # columns: x0 (free, unshifted), x1' = 4 - x1 (column and cost negated), x2' = x2 - 1.5 (u = 4.5), the slack of the inequality row
    assert np.array_equal(F.A.toarray(), [[1.0, -2.0, -1.0, 1.0], [3.0, 1.0, 4.0, 0.0]])
    assert np.array_equal(F.b.ravel(), [7.0 - 2.0 * 4.0 + 1.5, 9.0 + 4.0 - 4.0 * 1.5])
    assert np.array_equal(F.c.ravel(), [2.0, 3.0, 5.0, 0.0]) and np.array_equal(F.u, [np.inf, np.inf, 4.5, np.inf])
    assert F.offset == -3.0 * 4.0 + 5.0 * 1.5 and F.free.tolist() == [0] and F.free.dtype == np.int32
    assert np.array_equal(F.sign, [1.0, -1.0, 1.0, 1.0]) and np.array_equal(F.keep, [0, 1, 2, 3]) and F.fixed.size == 0 and F.n == 3
    # round trip: x' -> x, and the objective and the rows agree
    xn = np.array([-2.5, 1.0, 0.5, 0.25])
    x = F.x_original(xn)
    assert np.array_equal(x, [-2.5, 3.0, 2.0])
    assert abs(float(F.c.ravel() @ xn) + F.offset - float(np.dot(c, x))) <= 1e-14
    assert np.allclose(F.A @ xn - F.b.ravel(), [Aineq[0] @ x + xn[3] - 7.0, Aeq[0] @ x - 9.0], atol=1e-14)
    assert np.array_equal(general_form._ray_native(F, [1.0, 2.0, 3.0, 4.0], primal=True), [1.0, -2.0, 3.0, 4.0])
    assert np.array_equal(general_form._ray_native(F, [1.0, 2.0, 3.0, 4.0]), [1.0, 2.0, 3.0, 4.0])


def test_native_form_without_the_option_is_unchanged():
    c, Aeq, beq = [1.0, 2.0, 3.0], np.array([[1.0, 1.0, 1.0]]), [4.0]
    a = general_form.native_form(c, Aeq=Aeq, beq=beq, lb=[0.0, 1.0, 2.0], ub=[np.inf, 5.0, 2.0])
    b = general_form.native_form(c, Aeq=Aeq, beq=beq, lb=[0.0, 1.0, 2.0], ub=[np.inf, 5.0, 2.0], free="native")
    for k in ("b", "c", "u", "offset", "keep", "fixed", "lb0", "n"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.A.toarray(), b.A.toarray()) and a.free.size == 0 and np.all(a.sign == 1) and a.fixed.tolist() == [2]
    with pytest.raises(ValueError, match="free variables are not supported"):
        general_form.native_form(c, Aeq=Aeq, beq=beq, lb=[-np.inf, 0.0, 0.0])
    with pytest.raises(ValueError, match="free must be"):
        general_form.native_form(c, Aeq=Aeq, beq=beq, free="yes")


def general_form_problem():
    """A constructed general-form LP with a unique, strictly complementary optimum: 7 variables -- x0 free, x1 in (-inf, 3] AT its
    bound, x2 >= 1.5 AT its (shifted) lower bound, x3 in [0, 2] and x4 >= 0 at 0, x5, x6 >= 0 basic -- two inequality rows (the first
    active, the second slack by 0.7) and two equality rows.  c = -Aineq^T lam - Aeq^T nu + r_lower - r_upper."""
    rng = np.random.default_rng(21)
    Aineq, Aeq = rng.standard_normal((2, 7)), rng.standard_normal((2, 7))
    x = np.array([-1.25, 3.0, 1.5, 0.0, 0.0, 0.8, 1.7])
    lb = np.array([-np.inf, -np.inf, 1.5, 0.0, 0.0, 0.0, 0.0])
    ub = np.array([np.inf, 3.0, np.inf, 2.0, np.inf, np.inf, np.inf])
    lam, nu = np.array([0.9, 0.0]), np.array([0.6, -1.1])
    r_lower = np.array([0.0, 0.0, 0.7, 1.2, 0.5, 0.0, 0.0])
    r_upper = np.array([0.0, 1.3, 0.0, 0.0, 0.0, 0.0, 0.0])
    c = -Aineq.T @ lam - Aeq.T @ nu + r_lower - r_upper
    return dict(c=c, Aineq=Aineq, bineq=Aineq @ x + np.array([0.0, 0.7]), Aeq=Aeq, beq=Aeq @ x, lb=lb, ub=ub, x_star=x, obj_star=float(c @ x),
                n_free=1, n_bounded=1)


def test_general_form_problem_through_the_host_loop():
    """native_form(free="native") of the constructed problem, solved by the float64 host loop, maps back to the constructed optimum."""
    P = general_form_problem()
    F = general_form.native_form(P["c"], Aeq=P["Aeq"], beq=P["beq"], Aineq=P["Aineq"], bineq=P["bineq"], lb=P["lb"], ub=P["ub"], free="native")
    assert F.free.tolist() == [0] and int(np.isfinite(F.u).sum()) == 1 and F.sign[1] == -1
    r = FL.solve64(F.A.toarray(), F.b, F.c, F.u, F.free, tol=1e-9)
    x = F.x_original(r["x"])
    assert r["converged"] and np.linalg.norm(x - P["x_star"]) <= 1e-6 * np.linalg.norm(P["x_star"])
    assert abs(r["objective"] + F.offset - P["obj_star"]) <= 1e-7


# ---- every ValueError -----------------------------------------------------------------------------------------------------------
def test_check_free_lp_and_rho():
    assert handle.check_free_lp(None, 5) is None and handle.check_free_lp([], 5) is None and handle.check_free_lp(np.zeros(5, dtype=bool), 5) is None
    idx = handle.check_free_lp([3, 1], 5)
    assert idx.dtype == np.int32 and idx.tolist() == [3, 1]
    assert handle.check_free_lp(np.array([True, False, True, False, False]), 5).tolist() == [0, 2]
    for bad, word in (([5], "free_lp: column index 5 out of range"), ([-1], "out of range"), ([1, 1], "free_lp: column index 1 is given twice"),
                      ([0.5], "free_lp must be column indices"), (np.ones(4, dtype=bool), "free_lp: the mask has 4 entries"),
                      (range(5), "free_lp: all 5 columns free")):
        with pytest.raises(ValueError, match=word):
            handle.check_free_lp(bad, 5)
    with pytest.raises(ValueError, match="free_lp: column 2 has the finite upper bound 4.0"):
        handle.check_free_lp([1, 2], 5, ub=[np.inf, np.inf, 4.0, 1.0, np.inf])
    with pytest.raises(ValueError, match="free_lp: column 1 is an LP free column, but the problem has a quadratic term"):
        handle.check_free_lp([1], 5, quad=np.array([0.0, 0.0, 1.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="free columns with curvature"):
        handle.check_free_lp([1], 5, free=[2])
    assert handle.check_free_rho(None) == 0.0 and handle.check_free_rho(-1.0) == 0.0 and handle.check_free_rho(0) == 0.0 and handle.check_free_rho(1e-6) == 1e-6
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="free_rho"):
            handle.check_free_rho(bad)
    assert _lib.FREE_LP_RHO_DEFAULT == 1e-8


def test_constructor_refusals_before_any_device():
    A, b, c, free, u, xs, ys, ss = FL.problem("8x20")
    bad = [(dict(free_lp=[20]), "out of range"), (dict(free_lp=free, quad=np.full(20, 0.5)), "quadratic term"),
           (dict(free_lp=free, lockstep=True), "a lockstep solver takes no LP free columns"),
           (dict(free_lp=free, detect_infeasibility=True), "detect_infeasibility=True takes no LP free columns"),
           (dict(free_lp=free, correctors=2), "correctors=2 takes no LP free columns"), (dict(free_lp=free, free_rho=np.nan), "free_rho"),
           (dict(free_lp=free, ub=np.where(np.arange(20) == free[0], 1.0, np.inf)), "column %d has the finite upper bound" % free[0])]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            ipm.IpmSolver(A, b, c, **kw)
        with pytest.raises(ValueError, match=word):
            ipm.solve_with_info(A, b, c, **{k: v for k, v in kw.items() if k != "lockstep"}) if "lockstep" not in kw else ipm.IpmSolver(A, b, c, **kw)


def test_batch_front_ends_refuse_the_option():
    for fn, args in ((batches.solve_lockstep, ([],)), (batch.solve_shard_lockstep, ([], [])), (batch.run_batch, ([],)), (batches.solve_small_batch, ([],))):
        with pytest.raises(ValueError, match="free_lp: .* takes no LP free columns"):
            fn(*args, free_lp=[1])
        assert inspect.signature(fn).parameters["free_lp"].default is None
    # the QP siblings' parameter lists are pinned by existing tests (as for `free`): they take no such keyword at all, and Python
    # itself refuses it
    for fn in (ipm.solve_small_qp_batch, ipm.solve_small_factor_qp_batch, ipm.solve_small_qp_batch_detect, ipm.solve_small_factor_qp_batch_detect):
        with pytest.raises(TypeError):
            fn([], free_lp=[1])


def test_general_form_value_errors():
    P = general_form_problem()
    kw = dict(Aeq=P["Aeq"], beq=P["beq"], Aineq=P["Aineq"], bineq=P["bineq"], lb=P["lb"], ub=P["ub"])
    with pytest.raises(ValueError, match='free="native" needs bounds="native"'):
        general_form.new_interior_sparse(P["c"], bounds="fold", free="native", **kw)
    with pytest.raises(ValueError, match="free must be"):
        general_form.new_interior_sparse(P["c"], bounds="native", free="split", **kw)
    with pytest.raises(ValueError, match="free variables are not supported"):
        general_form.native_problem(P["c"], **kw)
    with pytest.raises(ValueError, match="native_problem: the problem has 1 free variables"):
        general_form.native_problem(P["c"], free="native", **kw)
    kw["lb"] = np.where(np.isinf(P["lb"]) & np.isinf(P["ub"]), 0.0, P["lb"])          # only the (-inf, ub] variable left: a batch problem again
    prob, F = general_form.native_problem(P["c"], free="native", **kw)
    assert F.free.size == 0 and F.sign[1] == -1 and len(prob) == 4


def test_signatures():
    for fn in (ipm.IpmSolver.__init__, ipm.solve, ipm.solve_with_info, ipm.interior_sparse):
        p = inspect.signature(fn).parameters
        assert p["free_lp"].default is None and p["free_rho"].default is None, fn
        named = [k for k, v in p.items() if v.kind is not inspect.Parameter.VAR_KEYWORD]
        assert named[-3:] == ["free_lp", "free_rho", "free_small"], fn
    p = inspect.signature(general_form.new_interior_sparse).parameters
    assert p["free"].default == "error" and p["free_rho"].default is None
    assert inspect.signature(general_form.native_form).parameters["free"].default == "error"
    assert hasattr(ipm.IpmSolver, "set_free_lp") and hasattr(ipm.IpmSolver, "free_lp_columns")


# ---- the ABI bindings -----------------------------------------------------------------------------------------------------------
def test_abi_bindings():
    lib = ipm.load_library()
    for name in ("ipm_set_free_lp_columns", "ipm_get_free_lp_columns", "ipm_debug_step_kernel_ex"):
        assert name in _lib.EXPORTS and getattr(lib, name).restype is C.c_int
    assert lib.ipm_set_free_lp_columns.argtypes[-1] is C.c_double and len(lib.ipm_get_free_lp_columns.argtypes) == 5
    assert lib.ipm_set_free_lp_columns(None, None, 0, 0.0) == -1 and b"ipm_set_free_lp_columns: NULL handle" in lib.ipm_last_error(None)
    assert lib.ipm_get_free_lp_columns(None, None, 0, None, None) == -1 and b"ipm_get_free_lp_columns: NULL handle" in lib.ipm_last_error(None)
    header = open(_lib.LIB_PATH.replace("interiorpointmethod_amd/libipm_hip.so", "include/ipm_hip.h")).read()
    assert "#define IPM_FREE_LP_RHO_DEFAULT 1e-8" in header
    assert "int ipm_set_free_lp_columns(ipm_handle* h, const int32_t* idx, int32_t count, double rho);" in header
    assert "int ipm_get_free_lp_columns(ipm_handle* h, int32_t* idx, int32_t cap, int32_t* count, double* rho);" in header


# ---- the variant tables with the fifth switch -----------------------------------------------------------------------------------
STEPS = ["prepare", "stop_test", "scaling", "direction", "mu_aff", "corrector_rhs", "update"]
STARTS = ["start_primal", "start_dual", "start_shift", "start_primal_correct", "start_dual_correct"]
START_IDS = {name: 11 + i for i, name in enumerate(STARTS)}          # IPM_STEP_START_PRIMAL = 11 (include/ipm_hip.h)


def _row_ex(step, b, d, q, f, l):
    lib = ipm.load_library()
    buf = C.create_string_buffer(128)
    twin = C.c_int32(-7)
    rc = lib.ipm_debug_step_kernel_ex(step, b, d, q, f, l, buf, 128, C.byref(twin))
    return rc, buf.value.decode(), twin.value


def _row(step, b, d, q, f):
    lib = ipm.load_library()
    buf = C.create_string_buffer(128)
    twin = C.c_int32(-7)
    rc = lib.ipm_debug_step_kernel(step, b, d, q, f, buf, 128, C.byref(twin))
    return rc, buf.value.decode(), twin.value


def test_the_new_class_by_hand():
    """Written out: each of the seven steps and the five start steps has one kernel for the plain and one for the bounded LP free
    class, none of them a lockstep twin."""
    for i, name in enumerate(STEPS):
        assert _row_ex(i, 0, 0, 0, 0, 1) == (0, name + "_free_lp_kernel", -1)
        assert _row_ex(i, 1, 0, 0, 0, 1) == (0, name + "_bounded_free_lp_kernel", -1)
    for name, i in START_IDS.items():
        assert _row_ex(i, 0, 0, 0, 0, 1) == (0, name + "_free_lp_kernel", -1)
        assert _row_ex(i, 1, 0, 0, 0, 1) == (0, name + "_bounded_free_lp_kernel", -1)
    # by hand, the spelling itself (not derived from the step's name)
    assert _row_ex(0, 1, 0, 0, 0, 1)[1] == "prepare_bounded_free_lp_kernel" and _row_ex(5, 0, 0, 0, 0, 1)[1] == "corrector_rhs_free_lp_kernel"
    assert _row_ex(14, 1, 0, 0, 0, 1)[1] == "start_primal_correct_bounded_free_lp_kernel"


def test_the_fifth_switch_is_legal_only_alone_or_with_bounds():
    for b in (0, 1):
        for d, q, f in ((1, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)):
            rc, _, _ = _row_ex(0, b, d, q, f, 1)
            assert rc == -1 and b"LP free columns" in ipm.load_library().ipm_last_error(None), (b, d, q, f)
        rc, _, _ = _row_ex(0, b, 0, 0, 1, 1)                       # free without quad stays the older refusal
        assert rc == -1 and b"free columns without a quadratic term" in ipm.load_library().ipm_last_error(None)
        for small in (7, 8, 9, 10):                                # IPM_STEP_SMALL .. IPM_STEP_SMALL_START_BATCH
            rc, _, _ = _row_ex(small, b, 0, 0, 0, 1)
            assert rc == -1 and b"one-workgroup path" in ipm.load_library().ipm_last_error(None)
    assert _row_ex(16, 0, 0, 0, 0, 1)[0] == -1 and _row_ex(-1, 0, 0, 0, 0, 1)[0] == -1


def test_without_the_fifth_switch_the_new_entry_answers_as_the_old_one():
    for step in range(16):
        for bits in range(16):
            b, d, q, f = bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1
            old, new = _row(step, b, d, q, f), _row_ex(step, b, d, q, f, 0)
            assert old[0] == new[0] and (old[0] != 0 or old == new), (step, bits, old, new)
            assert old[0] == (-1 if f and not q else 0)
    # and the old entry's answers for the LP classes are what they were (the rows the new class sits beside)
    assert _row(0, 0, 0, 0, 0)[1] == "LS_PREPARE" and _row(0, 1, 0, 0, 0)[1] == "LS_PREPARE_BND" and _row(2, 0, 0, 0, 0) == (0, "scaling_kernel", -1)
    assert _row(3, 0, 0, 1, 1) == (0, "direction_free_kernel", -1) and _row(11, 1, 0, 1, 1) == (0, "start_primal_bounded_kernel", -1)
