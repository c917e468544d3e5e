"""Free columns with curvature on the CPU, before tests/test_gpu_free_qp.py holds the device to the same oracle:

  * the float64 restatement of one iteration with free columns (tests/free_qp_oracle.py) agrees with the longdouble one to the 1e-12
    that tests/test_qp_oracle_host.py uses, on every case the GPU tests use;
  * with an empty free set the oracle IS qp_oracle.iterate, bit for bit;
  * the directions satisfy the unreduced Newton system, where the row of a free column is A^T dy - g dx = -r_c and ds = 0;
  * the float64 loop reaches the constructed optimum of workloads.factor_qp at every shape the GPU tests solve;
  * factor_qp_form entry for entry on a 2 x 3, k = 1 problem written out by hand, sparse and dense alike; at the optimum of the
    augmented problem x[:n] satisfies the KKT conditions of the ORIGINAL dense-Q problem;
  * every ValueError of the Python front ends, raised before any device is touched;
  * the new symbols are declared, exported and bound; with a NULL handle they return -1 and leave a text that names them.

Bounds.  1e-12 and the Newton rows: as in test_qp_oracle_host.py (observed here: at most 4.0e-15 and 2.2e-16).  Constructed optimum:
1e-7 as there for x (the stop test leaves x_j s_j <= 1e-8 with s* >= 0.5); observed 1.7e-12 .. 8.7e-11.  y and t follow x through
A and F: the same 1e-7 (observed at most 1.2e-9).  KKT of the original problem: the stop test's own 1e-8 relative residuals, a
factor 10 for moving from the augmented norm to the original one.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batch, batches, handle, workloads

import free_qp_oracle as FO
import iteration_oracle as IO
import qp_oracle as Q

LD = IO.LD
VECTORS = ("dxa", "dya", "dsa", "dwa", "dza", "atdya", "dx", "dy", "ds", "dw", "dz", "atdy", "xn", "yn", "sn", "wn", "zn", "atyn", "rc", "theta",
           "va", "qa", "v", "q")
SCALARS = ("alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "mu", "mu_aff", "sigma", "gap", "objective", "rp_norm", "rd_norm")


# ---- the oracle held to itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FO.ITER_CASES))
def test_float64_restatement_agrees_with_longdouble(name):
    case, g, free = FO.get(name)
    o, f = FO.oracle(name), FO.iterate(case, g, free, T=np.float64)
    errs = {k: IO.rel(f[k], o[k]) for k in VECTORS}
    errs.update({k: float(abs(LD(f[k]) - o[k]) / abs(o[k])) for k in SCALARS if k not in ("rp_norm", "rd_norm")})
    errs["rp_norm"] = IO.residual_rel(f["rp_norm"], o["rp_norm"], o["b_norm"])
    errs["rd_norm"] = IO.residual_rel(f["rd_norm"], o["rd_norm"], o["c_norm"])
    for k in sorted(errs):
        print("HOST64 %s %s %.3e" % (name, k, errs[k]))
    bad = {k: v for k, v in errs.items() if not v <= 1e-12}
    assert not bad, (name, bad)
    assert o["alpha_p"] == o["alpha_d"] and o["alpha_aff_p"] == o["alpha_aff_d"]
    # the preconditions of the case: curvature and no bound on the free columns, a sigma to compare with, s = 0 throughout
    fm = FO.free_mask(free, case.n)
    assert np.all(g[fm] > 0) and not case.U[fm].any() and o["sigma"] > 1e-6 and 0 < o["alpha_p"] < 1
    for k in ("dsa", "ds", "sn", "qa", "q"):
        assert np.all(np.asarray(o[k])[fm] == 0), k
    assert np.array_equal(o["theta"][fm], 1 / g[fm].astype(LD))


def test_cases_cover_what_they_claim():
    case, g, free = FO.get("40x600b")
    assert set(free.tolist()) == {0, 255, 256, 599} and case.x[255] == 0.0 and case.x[256] < 0 and case.bounded
    case, g, free = FO.get("40x600b-interleaved")
    U = case.U
    assert all(U[j - 1] and U[j + 1] for j in free.tolist()) and case.w[free[3] - 1] == 1e-2
    case, g, free = FO.get("5x50-all-but-one")
    assert free.shape[0] == case.n - 1
    case, g, free = FO.get("sparse/8x16500")
    assert case.n > 64 * 256 and (free >= 64 * 256).sum() >= 3 and (free < 64 * 256).sum() >= 2
    assert np.count_nonzero(case.A) < 4 * case.n
    case, g, free = FO.get("1x2")
    assert (case.m, case.n, free.tolist()) == (1, 2, [1])


@pytest.mark.parametrize("name", ["dense/400x520b", "dense/520x600", "sparse/130x300b"])
def test_empty_free_set_is_the_qp_oracle(name):
    case, g = Q.get(name)
    for T in (LD, np.float64):
        q = Q.iterate(case, g, T=T)
        f = FO.iterate(case, g, None, T=T)
        for k in set(VECTORS + SCALARS + ("b_norm", "c_norm", "aty", "rb", "ru", "r3c", "r4c")) - {"theta", "va", "qa", "v", "q"}:
            assert np.array_equal(np.asarray(f[k]), np.asarray(q[k])), (name, T, k)


@pytest.mark.parametrize("name", sorted(FO.ITER_CASES))
def test_newton_equations_hold(name):
    case, g, free = FO.get(name)
    o = FO.oracle(name)
    fm = FO.free_mask(free, case.n)
    nf = ~fm
    A = case.A.astype(LD)
    g = g.astype(LD)
    x, w, z = (np.asarray(v, dtype=LD) for v in (case.x, case.w, case.z))
    s = np.where(fm, LD(0), np.asarray(case.s, dtype=LD))
    U = case.U
    for tag, (dx, dy, ds, dw, dz), r3, r4 in (("aff", [o[k] for k in ("dxa", "dya", "dsa", "dwa", "dza")], x * s, w * z),
                                               ("cor", [o[k] for k in ("dx", "dy", "ds", "dw", "dz")], o["r3c"], o["r4c"])):
        atdy = dy @ A
        rows = {
            "primal": (A @ dx + o["rb"], [A @ dx, o["rb"]]),
            "dual": ((atdy + ds - dz - g * dx + o["rc"])[nf], [atdy[nf], ds[nf], dz[nf], (g * dx)[nf], o["rc"][nf]]),
            "dual-free": ((atdy - g * dx + o["rc"])[fm], [atdy[fm], (g * dx)[fm], o["rc"][fm]]),
            "xs": ((s * dx + x * ds + r3)[nf], [(s * dx)[nf], (x * ds)[nf], r3[nf]]),
            "bound": ((dx + dw + o["ru"])[U], [dx[U], dw[U], o["ru"][U]]),
            "wz": ((z * dw + w * dz + r4)[U], [(z * dw)[U], (w * dz)[U], r4[U]]),
        }
        for row, (res, terms) in rows.items():
            if res.size == 0:
                continue
            scale = max(float(np.abs(t).max()) for t in terms)
            err = float(np.abs(res).max()) / scale
            print("NEWTON %s %s %s %.3e" % (name, tag, row, err))
            assert err <= 1e-12, (name, tag, row, err)
        assert np.all(ds[fm] == 0) and np.all(dw[fm] == 0) and np.all(dz[fm] == 0)
    # the free row's residual carries no s: r_c = A^T y - c - g x there
    y = np.asarray(case.y, dtype=LD)
    assert np.array_equal(o["rc"][fm], ((y @ A) + LD(0) - LD(0) - np.asarray(case.c, dtype=LD) - g * x)[fm])


@pytest.mark.parametrize("name", sorted(FO.SOLVE_PROBLEMS))
def test_float64_loop_reaches_the_constructed_optimum(name):
    r = FO.host_loop(name)
    print("LOOP64 %s iterations %d x_err %.3e y_err %.3e t_err %.3e" % (name, r["iterations"], r["x_err"], r["y_err"], r["t_err"]))
    assert r["converged"] and r["iterations"] <= 30
    assert r["x_err"] <= 1e-7 and r["y_err"] <= 1e-7 and r["t_err"] <= 1e-7
    A, b, c, g, F, u, xs, ys = FO.problem(name)
    n = A.shape[1]
    assert np.all(r["s"][n:] == 0)                                             # the free columns never grew an s


def test_workload_builder():
    with pytest.raises(AssertionError):
        workloads.factor_qp(400, 520, 4, 0)                                    # 0.75 * 520 = 390 < 1.25 * 400 active columns
    A, b, c, g, F, u, xs, ys = workloads.factor_qp(60, 150, 4, 0, bounded=True)
    assert F.shape == (150, 4) and u is not None and np.all(xs <= u) and np.any(xs == u) and np.all(g > 0)
    assert np.array_equal(b, A @ xs)
    assert workloads.factor_qp(3, 20, 2, 7)[5] is None


# ---- factor_qp_form ---------------------------------------------------------------------------------------------------------------
def test_factor_qp_form_by_hand():
    A = np.array([[1.0, 2.0, 0.0], [0.0, -1.0, 3.0]])
    b, c, g = np.array([4.0, 5.0]), np.array([1.0, -1.0, 0.5]), np.array([0.0, 2.0, 0.25])
    F = np.array([[0.5], [-1.5], [2.0]])
    u = np.array([np.inf, 7.0, np.inf])
    want_A = np.array([[1.0, 2.0, 0.0, 0.0], [0.0, -1.0, 3.0, 0.0], [0.5, -1.5, 2.0, -1.0]])
    for As in (A, sparse.csc_matrix(A), sparse.csr_matrix(A)):
        A_, b_, c_, g_, u_, free = ipm.factor_qp_form(As, b, c, g, F, u)
        assert sparse.issparse(A_) == sparse.issparse(As)
        if sparse.issparse(A_):
            assert A_.format == "csc"
        assert np.array_equal(A_.toarray() if sparse.issparse(A_) else A_, want_A)
        assert np.array_equal(b_, [4.0, 5.0, 0.0]) and np.array_equal(c_, [1.0, -1.0, 0.5, 0.0])
        assert np.array_equal(g_, [0.0, 2.0, 0.25, 1.0]) and np.array_equal(u_, [np.inf, 7.0, np.inf, np.inf])
        assert free.dtype == np.int32 and free.tolist() == [3]
    A_, b_, c_, g_, u_, free = ipm.factor_qp_form(A, b, c, None, F)            # g = None: zeros; no bounds: None
    assert np.array_equal(g_, [0.0, 0.0, 0.0, 1.0]) and u_ is None
    from interiorpointmethod_amd import solver
    assert solver.factor_qp_form is ipm.factor_qp_form and solver.solve_factor_qp is ipm.solve_factor_qp


@pytest.mark.parametrize("bad,match", [
    (dict(F=np.ones((3, 0))), "k >= 1"), (dict(F=np.ones((2, 1))), "n x k"), (dict(F=np.ones(3)), "n x k"),
    (dict(F=np.array([[1.0], [np.nan], [0.0]])), "finite"), (dict(g=np.array([1.0, -1.0, 0.0])), "quad"),
    (dict(g=np.ones(2)), "entries"), (dict(b=np.ones(3)), "b has"), (dict(c=np.ones(2)), "c has"), (dict(c=np.array([1.0, np.inf, 0.0])), "finite"),
    (dict(ub=np.ones(2)), "ub has"), (dict(ub=np.array([1.0, -1.0, np.inf])), "ub must"),
])
def test_factor_qp_form_refuses(bad, match):
    kw = dict(A=np.array([[1.0, 2.0, 0.0], [0.0, -1.0, 3.0]]), b=np.ones(2), c=np.ones(3), g=np.ones(3), F=np.ones((3, 1)), ub=None)
    kw.update(bad)
    with pytest.raises(ValueError, match=match):
        ipm.factor_qp_form(kw["A"], kw["b"], kw["c"], kw["g"], kw["F"], kw["ub"])
    for name in ("quad", "free"):                                              # solve_factor_qp builds both itself
        with pytest.raises(ValueError, match=name):
            ipm.solve_factor_qp(kw["A"], np.ones(2), np.ones(3), np.ones((3, 1)), **{name: None})


@pytest.mark.parametrize("name", ["3x20k2", "40x130k8b", "200x520k16"])
def test_augmented_optimum_is_the_original_problems(name):
    """At the host loop's optimum of the augmented problem, x[:n], y[:m], s[:n] (z[:n]) satisfy the KKT conditions of
    min c.x + 1/2 x.Q x with the DENSE Q = diag(g) + F F^T."""
    A, b, c, g, F, u, xs, ys = FO.problem(name)
    m, n = A.shape
    r = FO.host_loop(name)
    x, y, s, z, w = r["x"][:n], r["y"][:m], r["s"][:n], r["z"][:n], r["w"][:n]
    Qd = np.diag(g) + F @ F.T
    stat = c + Qd @ x - A.T @ y - s + z
    assert np.linalg.norm(stat) <= 1e-7 * (1 + np.linalg.norm(c)), np.linalg.norm(stat)
    assert np.linalg.norm(A @ x - b) <= 1e-7 * (1 + np.linalg.norm(b))
    assert x.min() >= 0 and s.min() >= 0 and x @ s + w @ z <= 1e-7
    if u is not None:
        U = np.isfinite(u)
        assert np.all(x[U] <= u[U] + 1e-9) and z.min() >= 0
    assert abs(c @ x + 0.5 * x @ Qd @ x - r["obj_star"]) <= 1e-7 * abs(r["obj_star"])
    # the multipliers of the rows F^T x - t = 0 are -t, the row of a free column: -y_t - g_t t = 0 with g_t = 1
    assert np.linalg.norm(r["y"][m:] + r["x"][n:]) <= 1e-7 * (1 + np.linalg.norm(r["x"][n:]))


# ---- the host checks of the Python front ends: ValueError before any device is touched ------------------------------------------------
def test_check_free():
    g = np.array([1.0, 0.0, 2.0, 0.5])
    assert handle.check_free(None, 4, g) is None and handle.check_free([], 4, g) is None
    assert handle.check_free(np.zeros(4, dtype=bool), 4, g) is None
    out = handle.check_free([2, 0], 4, g)
    assert out.dtype == np.int32 and out.tolist() == [2, 0]
    assert handle.check_free(np.array([True, False, False, True]), 4, g).tolist() == [0, 3]
    assert handle.check_free((3,), 4, g, np.array([1.0, 2.0, 3.0, np.inf])).tolist() == [3]
    for free, kw, match in (([4], {}, "index 4 out of range"), ([-1], {}, "index -1 out of range"), ([0, 2, 0], {}, "index 0 is given twice"),
                            ([1], {}, "column 1 has no quadratic term"), ([0], dict(quad=None), "column 0 has no quadratic term"),
                            ([0], dict(ub=np.array([3.0, np.inf, np.inf, np.inf])), "column 0 has the finite upper bound"),
                            ([0], dict(ub=np.array([np.inf, np.inf])), "ub has 2 entries"),
                            (np.ones(3, dtype=bool), {}, "mask has 3 entries"), ([0.5], {}, "indices"), ("ab", {}, "indices"),
                            ([0, 2, 3, 1], dict(quad=np.ones(4)), "no complementarity pair")):
        with pytest.raises(ValueError, match=match):
            handle.check_free(free, 4, kw.get("quad", g), kw.get("ub"))


def test_front_ends_refuse_before_any_device(monkeypatch):
    """IpmSolver, solve, solve_with_info, interior_sparse and solve_factor_qp raise ValueError naming the column, and the batch front
    ends raise when handed the option; no library call is made (load is patched to fail)."""
    def no_device(*a, **k):
        raise AssertionError("a device was about to be touched")
    monkeypatch.setattr(_lib, "load", no_device)
    A, b, c, g, u, xs, ys = workloads.separable_qp(5, 20, 1, bounded=True)
    j_b = int(np.flatnonzero(np.isfinite(u))[0])
    j_f = int(np.flatnonzero(~np.isfinite(u))[0])
    g0 = g.copy()
    g0[j_f] = 0.0
    for fn in (ipm.IpmSolver, ipm.solve, ipm.solve_with_info, ipm.interior_sparse):
        if fn is not ipm.interior_sparse:                                      # (which has no ub keyword)
            with pytest.raises(ValueError, match="column %d has the finite upper bound" % j_b):
                fn(A, b, c, ub=u, quad=g, free=[j_b])
        with pytest.raises(ValueError, match="column %d has no quadratic term" % j_f):
            fn(A, b, c, quad=g0, free=[j_f])
        with pytest.raises(ValueError, match="column %d has no quadratic term" % j_f):
            fn(A, b, c, free=[j_f])
        with pytest.raises(ValueError, match="out of range"):
            fn(A, b, c, quad=g, free=[20])
    for kw, match in ((dict(detect_infeasibility=True), "detect_infeasibility"), (dict(correctors=1), "correctors"), (dict(lockstep=True), "lockstep")):
        with pytest.raises(ValueError, match=match):
            ipm.IpmSolver(A, b, c, quad=g, free=[j_f], **kw)
    for kw, match in ((dict(detect_infeasibility=True), "detect_infeasibility"), (dict(correctors=1), "correctors"), (dict(start="mehrotra"), "mehrotra")):
        with pytest.raises(ValueError, match=match):
            ipm.solve_with_info(A, b, c, quad=g, free=[j_f], **kw)
    for call in (lambda: batches.solve_lockstep([], free=[j_f]), lambda: batch.solve_shard_lockstep([(A, b, c)], [0], free=[j_f]),
                 lambda: batch.run_batch([(A, b, c)], free=np.arange(20) == j_f), lambda: batches.solve_small_batch([(A, b, c)], free=[j_f])):
        with pytest.raises(ValueError, match="takes no free columns"):
            call()
    # solve_small_qp_batch's parameter list is pinned (tests/test_qp_small_cases_host.py::test_front_end_signatures), so it has no
    # `free` keyword to refuse with a ValueError: Python refuses the call itself, and nothing is dropped either
    with pytest.raises(TypeError, match="free"):
        batches.solve_small_qp_batch([(A, b, c, g)], free=[j_f])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ipm_hip.h")).read()
    lib = ipm.load_library()
    for name in ("ipm_set_free_columns", "ipm_get_free_columns"):
        assert "int %s(ipm_handle* h" % name in header and name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    k = C.c_int32(-7)
    assert lib.ipm_set_free_columns(None, None, 0) == -1 and b"ipm_set_free_columns" in lib.ipm_last_error(None)
    assert lib.ipm_get_free_columns(None, None, 0, C.byref(k)) == -1 and b"ipm_get_free_columns" in lib.ipm_last_error(None)
    assert k.value == -7
