"""Small factor-model QPs in the one-workgroup kernel (IPM_FLAG_SMALL_FREE, IpmSolver(quad=g, free=..., free_small=True);
DESIGN.md 4-U): the Free instantiations of small_lp_body (csrc/small_lp.h), alone and in ipm_solve_small_batch, and the front end
solve_small_factor_qp_batch.

Every handle of parts 1 to 4 is a CSC handle created with free_small=True, and schedule()["fused_small"] == 1 is asserted for it.

1. One iteration against the longdouble oracle of tests/free_qp_oracle.py on the cells of tests/small_free_cases.py.
   (a) iterate(0) is the kernel's residual pass and stop test alone: r_c, d, v, q of residual_cols (ipm_debug_get_column_vector), element
       by element, q == 0 and d == 1 / g exactly on the free columns, and mu, the gap, the objective and both residual norms.
   (b) test_gpu_free_qp.check_free_iteration, unchanged: its iterate(1) is the new kernel (step lengths, mu, sigma, the updated state
       with s == 0 exactly on the free columns -- the kernel stores ds = 0 there and never adds to s --, the statistics and the history
       record with the pair count n - n_free + |U|); its newton_direction runs the multi-kernel Free kernels on the same handle (both
       directions, ds == 0 exactly on the free columns).
   Bounds: test_gpu_iteration_edges._bound, unchanged; r_c, d, v, q get its floor, 1e-12, as in tests/test_gpu_free_qp.py.
   (c) iterate(3) in one launch == three launches of iterate(1), bit for bit.
2. Whole solves of workloads.factor_qp through solve_factor_qp(..., free_small=True) by the criteria of part 3 of
   tests/test_gpu_small_qp.py (test_gpu_qp.check_solve): status 1, iterations within 2 of the float64 host loop's, the stop test
   re-evaluated in longdouble on the augmented problem within 2 tol, x and the ORIGINAL objective within max(1e-9, 100 x the host
   loop's error); the same x under the same bound against the multi-kernel solve.  m + k = 129 lands on the multi-kernel path.
3. Invariants: bitwise repeat; the flag without a set is the quad_small handle bit for bit; a set made and cleared equals never set;
   the set before A and after A; scale="ruiz" against the host-prescaled problem.
4. Batch: two handles of each of the eight variants in one shuffled call, one free-variant problem with duplicated rows in the shifted
   second round, 300 free-variant QPs on 256 compute units, solve_small_factor_qp_batch against solve_factor_qp -- each bit for bit.
5. Refusals, each leaving the handle usable.

Observed maxima on MI355X (first run of this file; every quantity stayed under its bound on that run, so no bound was replaced), per
quantity over the eight cells of part 1, and the cell that gave it (OBSERVED_SMALL_FREE below):
    the residual pass alone (iterate(0)): r_c 1.8e-16, v 2.1e-16, gap 1.7e-16, mu 1.8e-16    factor/128x300        d 5.8e-17    stride/5x600b
        q 1.6e-16, rd_norm 1.5e-16    1x2        rp_norm 3.3e-16    5x50-all-but-one        objective 3.6e-16    factor/17x40
    ds 5.2e-15, dsa 3.4e-15, s 3.6e-15, x 8.6e-16, y 1.5e-15, A^T y 1.6e-15                              5x50-all-but-one
    dxa 1.7e-15, dya 1.2e-15, dy 1.3e-15, A^T dya 8.0e-16, corrector v 9.5e-16                            factor/128x300
    sigma 2.8e-15, corrector q 2.4e-15, mu_aff 1.1e-15, alpha_aff_p/d 1.0e-15, A^T dy 9.2e-16            factor/16x40
    dx 1.5e-15    factor/17x40        dw 7.0e-16, dz 9.3e-16, z 3.3e-16, alpha_p/d 4.4e-16    between/17x40b        w 1.4e-16    stride/5x600b
Whole solves (OBSERVED_SOLVES): the device's iteration counts equal the host loop's on both paths (11, 12, 11) and its errors against
the constructed optimum equal the host loop's to three digits; x of the one-workgroup solve and of the multi-kernel solve differ by
9.4e-17, 1.4e-15, 2.7e-15.  Device time of the lone solves, one-workgroup against multi-kernel: 0.41 / 1.12 ms at 1 x 64 k = 8,
4.37 / 1.86 ms at 50 x 130 k = 10, 46.8 / 2.3 ms at 100 x 300 k = 28 (one workgroup forms the 2.5 million terms of the product list).
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, workloads
from interiorpointmethod_amd.factor_qp import factor_qp_solution

import equilibrate_oracle as EO
import free_qp_oracle as FO
import iteration_oracle as IO
import qp_oracle as Q
import qp_small_cases as QS
import small_free_cases as SF
from test_gpu_free_qp import _bound_free, _record_bytes, check_free_iteration
from test_gpu_iteration_edges import _assert_all, _srel
from test_gpu_small_batch import assert_same, collect, duplicated_rows_lp, synthetic

pytestmark = pytest.mark.gpu
TOL = FO.TOL

# the maxima of the first run of this file on an MI355X over the cells of part 1, for the record (the bounds are _bound's and FLOOR, not
# multiples of these; every quantity stayed under its bound on that run, so no bound was replaced)
OBSERVED_SMALL_FREE = {"res.rc": 1.8e-16, "res.d": 5.8e-17, "res.v": 2.1e-16, "res.q": 1.6e-16, "res.mu": 1.8e-16, "res.gap": 1.7e-16, "res.objective": 3.6e-16,
                       "res.rp_norm": 3.3e-16, "res.rd_norm": 1.5e-16, "dxa": 1.7e-15, "dsa": 3.4e-15, "ATdya": 8.0e-16, "dya": 1.2e-15, "dx": 1.5e-15,
                       "ds": 5.2e-15, "dw": 7.0e-16, "dz": 9.3e-16, "ATdy": 9.2e-16, "dy": 1.3e-15, "x": 8.6e-16, "s": 3.6e-15, "w": 1.4e-16, "z": 3.3e-16,
                       "ATy": 1.6e-15, "y": 1.5e-15, "alpha_aff_p": 1.0e-15, "alpha_aff_d": 1.0e-15, "alpha_p": 4.4e-16, "alpha_d": 4.4e-16, "mu": 1.8e-16,
                       "mu_aff": 1.1e-15, "sigma": 2.8e-15, "gap": 1.7e-16, "objective": 3.6e-16, "rp_norm": 3.3e-16, "rd_norm": 1.5e-16, "rc": 1.3e-16,
                       "d": 5.8e-17, "v": 9.5e-16, "q": 2.4e-15}
# whole solves: name -> (iterations = the host loop's, on both paths; x error; the host loop's x error)
OBSERVED_SOLVES = {"1x64k8b": (11, 4.471e-11, 4.471e-11), "50x130k10b": (12, 4.468e-12, 4.468e-12), "100x300k28": (11, 2.273e-11, 2.273e-11)}


def _small(A, b, c, ub=None, quad=None, free=None, **kw):
    """A CSC handle with the flag, on the one-workgroup path."""
    sv = ipm.IpmSolver(sparse.csc_matrix(A), b, c, ub=ub, quad=quad, free=free, free_small=True, **kw)
    assert sv.schedule()["fused_small"] == 1 and sv.sparse and sv.free_small, sv.schedule()
    return sv


def _cell(name, **kw):
    case, g, free = SF.get(name)
    sv = _small(case.A, case.b, case.c, ub=case.ub(), quad=g, free=free, **kw)
    assert (sv.m, sv.n) == (case.m, case.n) and sv.bounded == int(case.U.sum()) and sv.free_columns().tolist() == list(free)
    return sv


def _bits(sv):
    return [v.tobytes() for v in sv.get_state() + (sv.get_bound_state() or ())]


def _collect(sv):
    """State and bound state as bytes, the history, the statistics without the clock."""
    return _bits(sv), sv.history(), {k: v for k, v in sv.stats.items() if k != "solve_ms"}


# ---- 1. one iteration against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SF.CELLS)
def test_one_iteration(name):
    case, g, free = SF.get(name)
    o = SF.oracle(name)
    fm = FO.free_mask(free, case.n)
    with _cell(name) as sv:
        sv.set_state(*case.state())
        st = sv.iterate(0)                                             # the residual pass and the stop test of the Free kernel, alone
        assert st["iterations"] == 0
        rc, d, v, q = (sv.debug_column_vector(k) for k in ("rc", "d", "v", "q"))
        assert np.all(q[fm] == 0) and np.array_equal(d[fm], 1.0 / g[fm]) and np.array_equal(v[fm], d[fm] * rc[fm])
        assert np.all(np.isfinite(rc)) and np.all(np.isfinite(v)) and np.all(np.isfinite(q))
        e = {"res.rc": IO.rel(rc, o["rc"]), "res.d": IO.rel(d, o["theta"]), "res.v": IO.rel(v, o["va"]), "res.q": IO.rel(q, o["qa"]),
             "res.mu": _srel(st["mu"], o["mu"]), "res.gap": _srel(st["gap"], o["gap"]), "res.objective": _srel(st["objective"], o["objective"]),
             "res.rp_norm": IO.residual_rel(st["rp_norm"], o["rp_norm"], o["b_norm"]), "res.rd_norm": IO.residual_rel(st["rd_norm"], o["rd_norm"], o["c_norm"])}
        _assert_all(name, e, {k: _bound_free(k) for k in e})
        check_free_iteration(name, sv, case, g, free, o)
        assert sv.schedule()["fused_small"] == 1


@pytest.mark.parametrize("name", ["stride/5x600b", "between/17x40b", "factor/128x300"])
def test_three_steps_at_once_equal_three_single_steps(name):
    case, g, free = SF.get(name)
    fm = FO.free_mask(free, case.n)
    out = []
    for steps in ((3,), (1, 1, 1)):
        with _cell(name) as sv:
            sv.set_state(*case.state())
            for k in steps:
                st = sv.iterate(k)
            hist = sv.history()
            assert len(hist) == 3 and st["iterations"] == 3
            out.append((_bits(sv), _record_bytes([st]), _record_bytes(hist)))
            x, y, s = sv.get_state()
            assert np.all(np.isfinite(x)) and np.all(s.ravel()[fm] == 0)
    assert out[0] == out[1]


# ---- 2. whole solves --------------------------------------------------------------------------------------------------------
def check_small_factor_solve(cell, name, x, y, s, info, path):
    A, b, c, g, F, u, xs, ys = SF.problem(name)
    ref = SF.host_loop(name)
    m, n = A.shape
    k = F.shape[1]
    x, y, s = x.ravel(), y.ravel(), s.ravel()
    assert info["status"] == 1, (cell, info["status"])
    assert info["factors"] == k and info["free"] == k and info["quadratic"] == n + k and info["quadratic_path"] == path, (cell, info["quadratic_path"])
    A_, b_, c_, g_, u_, free = ipm.factor_qp_form(A, b, c, g, F, u)
    xa, ya, sa = np.concatenate([x, info["t"]]), np.concatenate([y, info["y_factor"]]), np.concatenate([s, np.zeros(k)])
    pad = (lambda v: None if v is None else np.concatenate([np.asarray(v).ravel(), np.zeros(k)]))
    rp, rd, gap = Q.stop_test_ld(A_, b_, c_, g_, u_, xa, ya, sa, pad(info.get("w")), pad(info.get("z")))
    original = lambda xv: float(c @ xv + 0.5 * (g * xv) @ xv + 0.5 * ((F.T @ xv) @ (F.T @ xv)))          # noqa: E731
    x_err = float(np.linalg.norm(x - xs) / np.linalg.norm(xs))
    obj_err = abs(info["objective"] - ref["obj_star"]) / abs(ref["obj_star"])
    host_obj_err = abs(original(ref["x"][:n]) - ref["obj_star"]) / abs(ref["obj_star"])
    print("OBS %s iterations %d (host %d) rp %.3e rd %.3e gap %.3e x_err %.3e (host %.3e) obj_err %.3e (host %.3e)"
          % (cell, info["iterations"], ref["iterations"], rp, rd, gap, x_err, ref["x_err"], obj_err, host_obj_err))
    assert ref["converged"] and ref["iterations"] <= SF.SOLVE_CAP - 2
    assert abs(info["iterations"] - ref["iterations"]) <= 2, (cell, info["iterations"], ref["iterations"])
    assert rp <= 2 * TOL and rd <= 2 * TOL and gap <= 2 * TOL, (cell, rp, rd, gap)
    assert x_err <= max(1e-9, 100 * ref["x_err"]), (cell, x_err, ref["x_err"])
    assert obj_err <= max(1e-9, 100 * host_obj_err), (cell, obj_err, host_obj_err)
    assert abs(info["objective"] - original(x)) <= 1e-13 * abs(original(x)), (cell, info["objective"])
    assert info["alpha_p"] == info["alpha_d"] and np.all(s >= 0) and np.all(x > 0)


@pytest.mark.parametrize("name", SF.SOLVE_NAMES)
def test_whole_solve(name):
    A, b, c, g, F, u, xs, ys = SF.problem(name)
    assert A.shape[0] + F.shape[1] <= 128
    As = sparse.csc_matrix(A)
    x, y, s, info = ipm.solve_factor_qp(As, b, c, F, g=g, ub=u, tol=TOL, max_iter=SF.SOLVE_CAP, free_small=True)
    assert x.shape == (A.shape[1], 1) and y.shape == (A.shape[0], 1) and s.shape == x.shape and info["t"].shape == (F.shape[1],)
    check_small_factor_solve(name + "/one-workgroup", name, x, y, s, info, "one-workgroup")
    xm, ym, sm, infom = ipm.solve_factor_qp(As, b, c, F, g=g, ub=u, tol=TOL, max_iter=SF.SOLVE_CAP)          # the default: the multi-kernel path
    check_small_factor_solve(name + "/multi-kernel", name, xm, ym, sm, infom, "multi-kernel")
    rel = float(np.linalg.norm(x - xm) / np.linalg.norm(xm))
    print("OBS %s one-workgroup against multi-kernel: x %.3e, device ms %.3f against %.3f" % (name, rel, info["solve_ms"], infom["solve_ms"]))
    assert rel <= max(1e-9, 100 * SF.host_loop(name)["x_err"]), (name, rel)


def test_one_row_too_many_takes_the_multi_kernel_path():
    A, b, c, g, F, u, xs, ys = SF.problem(SF.BEYOND)
    assert A.shape[0] + F.shape[1] == 129
    A_, b_, c_, g_, u_, free = ipm.factor_qp_form(sparse.csc_matrix(A), b, c, g, F, u)
    with ipm.IpmSolver(A_, b_, c_, ub=u_, quad=g_, free=free, free_small=True) as sv:
        assert sv.schedule()["fused_small"] == 0 and sv.free_small and sv.m == 129
        sv.init_state(1.0)
        st = sv.solve(tol=TOL, max_iter=SF.SOLVE_CAP)
        x = sv.get_state()[0].ravel()[:A.shape[1]]
    ref = SF.host_loop(SF.BEYOND)
    assert st["status"] == 1 and abs(st["iterations"] - ref["iterations"]) <= 2
    assert np.linalg.norm(x - xs) / np.linalg.norm(xs) <= max(1e-9, 100 * ref["x_err"])


# ---- 3. invariants ----------------------------------------------------------------------------------------------------------
INVARIANT = "50x130k10b"


def _augmented(name=INVARIANT):
    A, b, c, g, F, u, xs, ys = SF.problem(name)
    return ipm.factor_qp_form(A, b, c, g, F, u)


def _run(quad="problem", free="problem", after=None, max_iter=SF.SOLVE_CAP, **kw):
    A_, b_, c_, g_, u_, fr = _augmented()
    with _small(A_, b_, c_, ub=u_, quad=g_ if isinstance(quad, str) else quad, free=fr if isinstance(free, str) else free, **kw) as sv:
        if after:
            after(sv)
        assert sv.schedule()["fused_small"] == 1
        sv.init_state(1.0)
        st = sv.solve(tol=TOL, max_iter=max_iter)
        return st, _collect(sv)


def test_bitwise_repeat():
    a, b = _run(), _run()
    assert a[0]["status"] == 1 and a[1] == b[1] and len(a[1][1]) == a[0]["iterations"]


def test_set_before_or_after_A():
    fr = _augmented()[5]
    before = _run()
    after = _run(free=None, after=lambda sv: sv.set_free(fr))
    term_last = _run(quad=None, free=None, after=lambda sv: (sv.set_free(fr), sv.set_quadratic(_augmented()[3])))
    assert before[0]["status"] == 1 and before[1] == after[1] and before[1] == term_last[1]


def test_the_flag_alone_and_a_cleared_set_change_nothing():
    """free_small without a set runs the Quad variant: the quad_small handle bit for bit; and so does a set made and cleared."""
    A, b, c, g, u, xs, ys = QS.problem("small/50x130bm")
    cols = np.flatnonzero((g > 0) & ~np.isfinite(u))[:3].astype(np.int32)
    assert cols.shape[0] == 3

    def run(after=None, **kw):
        with ipm.IpmSolver(sparse.csc_matrix(A), b, c, ub=u, quad=g, **kw) as sv:
            assert sv.schedule()["fused_small"] == 1
            if after:
                after(sv)
            assert sv.free_columns().shape[0] == 0
            sv.init_state(1.0)
            sv.solve(tol=TOL, max_iter=40)
            return _collect(sv)
    ref = run(quad_small=True)
    assert ref[2]["status"] == 1
    assert run(free_small=True) == ref
    assert run(free_small=True, quad_small=True) == ref
    assert run(free_small=True, after=lambda sv: (sv.set_free(cols), sv.set_free(None))) == ref
    with ipm.IpmSolver(sparse.csc_matrix(A), b, c, ub=u, quad=g, free=cols, free_small=True) as sv:      # (and the set does change the trajectory)
        assert sv.schedule()["fused_small"] == 1
        sv.init_state(1.0)
        sv.solve(tol=TOL, max_iter=40)
        assert _collect(sv)[1] != ref[1]


def test_equilibration_equals_the_prescaled_problem():
    """The rule of tests/test_gpu_equilibrate.py on the Free variants: scale="ruiz" is bit-identical, after unscaling, to an unscaled
    handle given the host-prescaled (R A C, R b, C c, u / C, g C^2); the marks are scale-free."""
    A, b, c, g, u, fr = _augmented()
    rng = np.random.default_rng(11)
    dr, dc = 10.0 ** rng.uniform(-3, 3, A.shape[0]), 10.0 ** rng.uniform(-3, 3, A.shape[1])
    A, b, c, g, u = dr[:, None] * A * dc[None, :], dr * b, dc * c, g * dc * dc, u / dc          # the same QP, badly scaled
    er, ec, changed = EO.ruiz(A, 16)
    assert 0 < changed < 16
    R, Cc = EO.factors(er, ec)
    A2, b2, c2, u2 = EO.prescale(A, b, c, u, er, ec)
    g2 = g * Cc * Cc
    out = []
    for scaled in (True, False):
        args, ub, gg = ((A, b, c), u, g) if scaled else ((A2, b2, c2), u2, g2)
        with _small(*args, ub=ub, scale="ruiz" if scaled else None, quad=gg, free=fr) as sv:
            if scaled:
                assert np.array_equal(sv.scaling()[1], Cc) and sv.scale_info["passes"] == changed
            assert np.array_equal(sv.quadratic(), gg) and sv.schedule()["fused_small"] == 1 and sv.free_columns().tolist() == list(fr)
            sv.init_state(1.0)
            st = sv.solve(tol=TOL, max_iter=40)
            out.append((st, sv.history(), sv.get_state(), sv.get_bound_state()))
    (st1, h1, (x1, y1, s1), wz1), (st2, h2, (x2, y2, s2), wz2) = out
    for k in st1:
        if k != "solve_ms":
            assert st1[k] == st2[k], (k, st1[k], st2[k])
    assert st1["iterations"] > 0 and h1 == h2
    Rc, Cv = R.reshape(-1, 1), Cc.reshape(-1, 1)
    assert np.array_equal(x1, Cv * x2) and np.array_equal(y1, Rc * y2) and np.array_equal(s1, s2 / Cv)
    assert np.array_equal(wz1[0], Cv * wz2[0]) and np.array_equal(wz1[1], wz2[1] / Cv)


# ---- 4. batch ---------------------------------------------------------------------------------------------------------------
def _make(P):
    return _small(P["A"], P["b"], P["c"], ub=P["ub"], quad=P.get("quad"), free=P.get("free"), detect_infeasibility=P["detect"])


def _solo(P, max_iter=200):
    with _make(P) as sv:
        sv.init_state(1.0)
        sv.solve(tol=1e-8, max_iter=max_iter)
        return collect(sv)


def _batch(Ps, max_iter=200):
    svs = []
    try:
        for P in Ps:
            svs.append(_make(P))
            svs[-1].init_state(1.0)
        ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=max_iter)
        return [collect(sv) for sv in svs]
    finally:
        for sv in svs:
            sv.close()


def _with_bounds(P, seed):
    ub = np.full(P["A"].shape[1], np.inf)
    ub[5:60:3] = 4.0                               # x0 < 1.5 everywhere: the strictly feasible point stays feasible
    return dict(P, ub=ub, name=P["name"] + "/ub")


def _with_term(P, seed):
    return dict(P, quad=Q.quad_diagonal(P["A"].shape[1], seed), name=P["name"] + "/quad")


def _with_free(P, cols):
    """Those columns of a problem with a term lose their sign constraint: they hold g > 0 and no bound."""
    cols = np.asarray(cols, dtype=np.int32)
    assert np.all(P["quad"][cols] > 0) and (P["ub"] is None or not np.isfinite(P["ub"][cols]).any())
    return dict(P, free=cols, name=P["name"] + "/free")


def test_all_eight_variants_in_one_call():
    """Two handles of every kernel variant in a shuffled order; one of the free-variant QPs has more than 5 % duplicated rows, so the
    second, shifted round of the call runs a Free kernel.  Nothing is compared approximately."""
    Ps = [synthetic(30, 80, seed=1), synthetic(100, 240, seed=2)]                                                  # plain
    Ps += [_with_bounds(synthetic(40, 100, seed=s), s) for s in (3, 4)]                                            # bounded
    Ps += [dict(synthetic(36, 90, seed=s), detect=True) for s in (5, 6)]                                           # detect
    Ps += [dict(_with_bounds(synthetic(40, 100, seed=s), s), detect=True) for s in (7, 8)]                         # bounded + detect
    Ps += [_with_term(synthetic(50, 130, seed=s), s) for s in (9, 10)]                                             # quad
    Ps += [_with_term(_with_bounds(synthetic(40, 100, seed=s), s), s) for s in (11, 12)]                           # bounded + quad
    dup = _with_free(_with_term(duplicated_rows_lp(), 9), [40, 42, 60])
    Ps += [_with_free(_with_term(synthetic(50, 130, seed=13), 13), [60, 64, 128]), dup]                            # free
    Ps += [_with_free(_with_term(_with_bounds(synthetic(40, 100, seed=s), s), s), [42, 46, 98]) for s in (15, 16)]  # bounded + free
    variant = lambda P: (P["ub"] is not None, bool(P["detect"]), P.get("quad") is not None, P.get("free") is not None)          # noqa: E731
    assert sorted(variant(P) for P in Ps) == sorted(2 * [(bd, dt, qd, fr) for bd in (False, True)
                                                         for dt, qd, fr in ((False, False, False), (True, False, False), (False, True, False), (False, True, True))])
    order = np.random.default_rng(7).permutation(len(Ps))
    assert not np.array_equal(order, np.arange(len(Ps)))
    Ps = [Ps[i] for i in order]
    refs = [_solo(P) for P in Ps]
    got = _batch(Ps)
    for P, g, r in zip(Ps, got, refs):
        assert_same(g, r, P["name"])
    shifted = {P["name"]: g["stats"]["auto_regularized"] for P, g in zip(Ps, got)}
    assert shifted[dup["name"]] == 1 and sum(shifted.values()) == 1, shifted
    for P, g in zip(Ps, got):
        if P.get("free") is not None:
            assert np.all(g["s"].ravel()[P["free"]] == 0) and g["stats"]["alpha_p"] == g["stats"]["alpha_d"], P["name"]
    assert sum(g["stats"]["status"] == 1 for g in got) >= 13, [g["stats"]["status"] for g in got]


def test_300_free_qps_equal_solo():
    """300 distinct 17 x 40 QPs with free columns in one call: more workgroups than the 256 compute units.  ALL are compared bit for bit."""
    Ps = [_with_free(_with_term(synthetic(17, 40, seed=20_000 + k), k), [20, 22, 38]) for k in range(300)]
    refs = [_solo(P, max_iter=100) for P in Ps]
    got = _batch(Ps, max_iter=100)
    for P, g, r in zip(Ps, got, refs):
        assert_same(g, r, P["name"])
    assert sum(g["stats"]["status"] == 1 for g in got) >= 150


def _same_record(info, ref, what):
    assert set(info) == set(ref) - {"setup_seconds", "solve_seconds", "teardown_seconds"}, what
    for k, v in info.items():
        if k in ("solve_ms", "setup_seconds", "solve_seconds", "teardown_seconds"):
            continue
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, ref[k]), (what, k)
        else:
            assert v == ref[k] or (v != v and ref[k] != ref[k]), (what, k, v, ref[k])


def test_python_front_end_equals_solve_factor_qp():
    problems, ub = [], []
    for m, n, k, seed, bounded in ((1, 64, 8, 7, True), (20, 60, 6, 3, False), (50, 130, 10, 7, True)):
        A, b, c, g, F, u, xs, ys = workloads.factor_qp(m, n, k, seed, bounded=bounded)
        problems.append((sparse.csc_matrix(A), b, c, F, g)); ub.append(u)
    A, b, c, g, u, xs, ys = QS.problem("small/17x40b")
    problems += [(sparse.csc_matrix(A), b, c, None, g), (A, b, c, np.zeros((A.shape[1], 0)), None)]      # F = None: a plain QP; k = 0 and no g: its LP
    ub += [u, u]
    got = ipm.solve_small_factor_qp_batch(problems, tol=TOL, ub=ub, max_iter=SF.SOLVE_CAP)
    assert len(got) == len(problems)
    for i, ((A, b, c, F, g), u, (x, y, s, info)) in enumerate(zip(problems, ub, got)):
        if F is not None and F.shape[1]:
            xr, yr, sr, ref = ipm.solve_factor_qp(A, b, c, F, g=g, ub=u, tol=TOL, max_iter=SF.SOLVE_CAP, free_small=True)
            assert info["quadratic_path"] == "one-workgroup" and info["factors"] == F.shape[1] == info["free"]
        else:
            # no factor: the plain solve on the same path, through the same translation (factors = 0, empty t and y_factor)
            m, n = A.shape
            raw = ipm.solve_with_info(sparse.csc_matrix(A), b, c, ub=u, quad=g, free_small=True, tol=TOL, max_iter=SF.SOLVE_CAP)
            xr, yr, sr, ref = factor_qp_solution(*raw, np.zeros((n, 0)), c, np.zeros(n) if g is None else g, m, n)
            assert info["quadratic_path"] == ("small" if g is not None else None) and info["free"] == 0 and info["factors"] == 0
            assert info["t"].shape == (0,) and abs(info["objective"] - info["objective_augmented"]) <= 1e-13 * abs(info["objective"])
        assert np.array_equal(x, xr) and np.array_equal(y, yr) and np.array_equal(s, sr), i
        if "w" in ref:
            assert info["w"].shape[0] == x.shape[0]
        _same_record(info, ref, i)
    assert all(r[3]["status"] == 1 for r in got[:4]), [r[3]["status"] for r in got]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def _small_problem():
    A, b, c, g, u, xs, ys = workloads.separable_qp(50, 130, 5)
    assert np.all(g > 0)
    return sparse.csc_matrix(A), b, c, g


def _usable(sv):
    sv.init_state(1.0)
    assert sv.solve(tol=TOL, max_iter=3)["iterations"] > 0


def test_with_the_flag_every_refusal_stays():
    A, b, c, g = _small_problem()
    n = c.shape[0]
    with pytest.raises(ValueError, match="detect_infeasibility"):         # detection: the host's refusal, before a handle exists
        ipm.IpmSolver(A, b, c, quad=g, free=[3], free_small=True, detect_infeasibility=True)
    with _small(A, b, c, detect_infeasibility=True) as sv:                 # ... and the library's own
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_DETECT_INFEASIBILITY") as ei:
            sv.set_free([3])
        assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
        _usable(sv)
    with pytest.raises(ValueError, match="correctors"):
        ipm.IpmSolver(A, b, c, quad=g, free=[3], free_small=True, correctors=1)
    with pytest.raises(ipm.IpmError, match="fused small-LP kernel"):
        ipm.IpmSolver(A, b, c, quad=g, free=[3], free_small=True, refine=1)
    with _small(A, b, c, quad=g, free=[3, 8]) as sv:
        with pytest.raises(ipm.IpmError, match="quadratic term") as ei:    # correctors: the term's reason comes first
            sv.set_correctors(1)
        assert ei.value.code == -1 and sv.correctors == 0
        with pytest.raises(ipm.IpmError, match="fused small-LP kernel") as ei:
            sv.set_refine(1)
        assert ei.value.code == -1 and sv.refine == 0
        with pytest.raises(ipm.IpmError, match="clear the free set first") as ei:      # clearing the term under a set
            sv.set_quadratic(None)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == int((g > 0).sum())
        g0 = g.copy()
        g0[8] = 0.0
        with pytest.raises(ipm.IpmError, match="needs g > 0"):             # ... or zeroing g on one free column
            sv.set_quadratic(g0)
        with pytest.raises(ValueError, match="all %d columns free" % n):   # the host's check of the indices
            sv.set_free(np.arange(n))
        every = np.arange(n, dtype=np.int32)
        code = sv._lib.ipm_set_free_columns(sv._h, every.ctypes.data_as(C.POINTER(C.c_int32)), n)      # ... and the library's own
        assert code == -1 and b"no complementarity pair" in sv._lib.ipm_last_error(sv._h)
        assert sv.free_columns().tolist() == [3, 8]
        with pytest.raises(ipm.IpmError, match="ipm_init_state_mehrotra") as ei:
            sv.init_state_mehrotra()
        assert ei.value.code == -1
        _usable(sv)
        assert sv.schedule()["fused_small"] == 1
    g1 = g.copy()
    g1[3] = 0.0
    with _small(A, b, c, quad=g1) as sv:                                   # g_j = 0 on a free column, the set after A
        with pytest.raises(ipm.IpmError, match="g = 0") as ei:
            sv.set_free([3])
        assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
        _usable(sv)
    with pytest.raises(ValueError, match="no quadratic term"):             # ... and before A, on the host
        ipm.IpmSolver(A, b, c, quad=g1, free=[3], free_small=True)
    ub = np.full(n, np.inf)
    ub[4] = 3.0
    with _small(A, b, c, ub=ub, quad=g) as sv:                             # a finite bound on a free column, the set after the bounds
        with pytest.raises(ipm.IpmError, match="finite upper bound") as ei:
            sv.set_free([4])
        assert ei.value.code == -1
        sv.set_free([6])
        assert sv.schedule()["fused_small"] == 1 and sv.free_columns().tolist() == [6]
        _usable(sv)
    with pytest.raises(ValueError, match="finite upper bound"):
        ipm.IpmSolver(A, b, c, ub=ub, quad=g, free=[4], free_small=True)


def test_batched_mehrotra_start_names_the_handle():
    A, b, c, g = _small_problem()
    svs = [_small(A, b, c), _small(A, b, c, quad=g, free=[3])]
    try:
        with pytest.raises(ipm.IpmError, match="handle 1 has free columns") as ei:
            ipm.init_small_batch_mehrotra(svs)
        assert ei.value.code == -1
        assert len(ipm.init_small_batch_mehrotra(svs[:1])) == 1            # without it the start runs
        for sv in svs:
            _usable(sv)
    finally:
        for sv in svs:
            sv.close()


def test_the_flag_needs_the_quadratic_flag_at_create():
    lib = _lib.load()
    for flags, ok in ((_lib.FLAG_SMALL_FREE, False), (_lib.FLAG_SMALL_FREE | _lib.FLAG_SMALL_QUADRATIC, True)):
        opts = _lib.Options()
        lib.ipm_default_options(C.byref(opts))
        opts.flags, opts.sparse_nnz = flags, 8
        h = C.c_void_p()
        code = lib.ipm_create(0, 3, 5, C.byref(opts), None, 0, None, C.byref(h))
        if ok:
            assert code == 0 and h.value
            lib.ipm_destroy(h)
        else:
            assert code == -1 and not h.value and b"IPM_FLAG_SMALL_FREE without IPM_FLAG_SMALL_QUADRATIC" in lib.ipm_last_error(None)


def test_without_the_flag_both_orders_behave_as_before():
    A, b, c, g = _small_problem()
    for kw in ({}, {"quad": g, "quad_small": True}):
        with ipm.IpmSolver(A, b, c, **kw) as sv:                                # A first: the one-workgroup path is taken ...
            assert sv.schedule()["fused_small"] == 1 and not sv.free_small
            with pytest.raises(ipm.IpmError, match="before A") as ei:           # ... and a free set then is refused
                sv.set_free([3])
            assert ei.value.code == -1 and sv.free_columns().shape[0] == 0
            _usable(sv)
    with ipm.IpmSolver(A, b, c, quad=g, quad_small=True, free=[3]) as sv:       # the set first: never the small path without free_small
        assert sv.schedule()["fused_small"] == 0 and sv.free_columns().tolist() == [3]
    with pytest.raises(ValueError, match="takes no free columns"):
        ipm.solve_small_batch([(A, b, c)], free=[3])
    with pytest.raises(TypeError):
        ipm.solve_small_qp_batch([(A, b, c, g)], free=[3])
