"""Small separable QPs in the one-workgroup kernel (IPM_FLAG_SMALL_QUADRATIC, IpmSolver(quad=g, quad_small=True)):
the Quad instantiations of small_lp_body (csrc/small_lp.h), alone and in ipm_solve_small_batch.

Every handle is a CSC handle created with quad_small=True, and schedule()["fused_small"] == 1 is asserted for it.

1. One iteration against the longdouble oracle of tests/qp_oracle.py on the cells of tests/qp_small_cases.py, through
   test_gpu_qp.check_qp_iteration: its iterate(1) is the new kernel, its newton_direction runs the multi-kernel Quad kernels on the
   same handle.  Bounds: test_gpu_iteration_edges._bound, unchanged (100 x the maxima observed there, floor 1e-12, under which
   tests/test_qp_small_cases_host.py holds the float64 restatement on every cell).  One step length, exactly.
2. Carry inside one launch: iterate(3) == three iterate(1) bit for bit, each step against the oracle started from the state read
   back before it.
3. Whole solves of workloads.separable_qp problems against qp_oracle.solve64, by test_gpu_qp.check_solve: iterations within 2 of the
   host loop's, the stop test in longdouble within 2 tol, x and objective within max(1e-9, 100 x the host loop's error).  50 x 130
   also against the unflagged multi-kernel handle: same status, iterations within 2, objective within 1e-9 relative.
4. Invariants: bitwise repeat; the flag without a term, and a term set and cleared, are the unflagged LP handle bit for bit;
   independence from check_every; scale="ruiz" against the host-prescaled problem (g C^2), the term set before and after the
   scaling; the term set before or after A.
5. Batch: all six kernel variants in one call, a duplicated-rows QP in the shifted second round, 300 QPs on 256 compute units, and
   solve_small_qp_batch with LPs mixed in -- each bit for bit its own solo solve.
6. Refusals: without the flag as before it existed; with it everything that was refused stays refused, each with its reason.

Observed maxima on MI355X (first run of this file; every quantity stayed under its bound on that run, so no bound was replaced), per
quantity over the seven cells of part 1, and the cell that gave it (OBSERVED_SMALL_QP below):
    dxa 2.2e-15, dsa 1.2e-15, dx 2.0e-15                                                                          tile/128x300
    dya 2.4e-15, A^T dya 1.2e-15, dy 3.3e-15, A^T dy 2.1e-15, ds 2.6e-15, alpha_aff_p/d 9.2e-16, sigma 1.9e-15      list/arrow
    dw 1.3e-15, dz 2.2e-15, x 7.4e-16, s 9.4e-16, w 5.3e-16, z 1.1e-15, y 1.6e-15, A^T y 1.2e-15, alpha_p/d 9.9e-16  tile/128x300b
    mu 2.7e-16, gap 2.8e-16    stride/20x513b        objective 6.4e-16    rows/24x64b        rp_norm 1.9e-16, rd_norm 2.1e-16    tile/1x2b
Part 2, over the three steps of both cells: at most 6.6e-15 (sigma, tile/17x40b); vectors at most 3.4e-15 (A^T y, tile/128x300).
Whole solves (OBSERVED_SOLVES): the device's iteration counts equal the host loop's (12, 12, 11, 11), and its errors against the
constructed optimum equal the host loop's to three digits.  A lone 50 x 130 solve took 12 iterations on both paths.
"""
import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import workloads

import equilibrate_oracle as EO
import qp_oracle as Q
import qp_small_cases as QS
from test_gpu_iteration_edges import HIST_SCALARS, _assert_all, _bound, measure
from test_gpu_qp import check_qp_iteration, check_solve
from test_gpu_small_batch import assert_same, collect, duplicated_rows_lp, synthetic

pytestmark = pytest.mark.gpu

# the maxima of the first run of this file on an MI355X over the cells of part 1, for the record (the bounds are _bound's, not multiples of these)
OBSERVED_SMALL_QP = {"dxa": 2.2e-15, "dsa": 1.2e-15, "ATdya": 1.2e-15, "dya": 2.4e-15, "dx": 2.0e-15, "ds": 2.6e-15, "dw": 1.3e-15, "dz": 2.2e-15,
                     "ATdy": 2.1e-15, "dy": 3.3e-15, "x": 7.4e-16, "s": 9.4e-16, "w": 5.3e-16, "z": 1.1e-15, "ATy": 1.2e-15, "y": 1.6e-15,
                     "alpha_aff_p": 9.2e-16, "alpha_aff_d": 9.2e-16, "alpha_p": 9.9e-16, "alpha_d": 9.9e-16, "mu": 2.7e-16, "sigma": 1.9e-15,
                     "gap": 2.8e-16, "objective": 6.4e-16, "rp_norm": 1.9e-16, "rd_norm": 2.1e-16}
OBSERVED_SOLVES = {"small/128x300bm": (12, 5.0e-12), "small/16x40m": (11, 2.1e-11), "small/17x40b": (11, 3.0e-11), "small/50x130bm": (12, 5.2e-12)}      # (iterations, x error)


def _small(A, b, c, ub=None, quad=None, **kw):
    """A CSC handle with the flag, on the one-workgroup path."""
    sv = ipm.IpmSolver(sparse.csc_matrix(A), b, c, ub=ub, quad=quad, quad_small=True, **kw)
    assert sv.schedule()["fused_small"] == 1 and sv.sparse and sv.quad_small, sv.schedule()
    return sv


def _cell(name, **kw):
    case, g = QS.get(name)
    sv = _small(case.A, case.b, case.c, ub=case.ub(), quad=g, **kw)
    assert (sv.m, sv.n) == (case.m, case.n) and sv.bounded == int(case.U.sum()) and sv.quadratic_nonzeros() == int((g > 0).sum())
    return sv


def _bits(sv):
    return [v.tobytes() for v in sv.get_state() + (sv.get_bound_state() or ())]


def _collect(sv):
    """State and bound state as bytes, the history, the statistics without the clock."""
    return _bits(sv), sv.history(), {k: v for k, v in sv.stats.items() if k != "solve_ms"}


# ---- 1. one iteration against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QS.CELLS)
def test_one_iteration(name):
    case, g = QS.get(name)
    with _cell(name) as sv:
        check_qp_iteration(name, sv, case, g, QS.oracle(name))
        assert sv.schedule()["fused_small"] == 1


# ---- 2. carry inside one launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tile/17x40b", "tile/128x300"])
def test_carry_inside_one_launch(name):
    """(a) iterate(3) in one launch == three launches of iterate(1), bit for bit.  (b) each of the three steps against the oracle
    started from the device state read back before the step: exact in float64, so no allowance for error growth."""
    case, g = QS.get(name)
    with _cell(name) as sv:
        sv.set_state(*case.state())
        st3 = sv.iterate(3)
        assert st3["iterations"] == 3
        one_launch = (_bits(sv), sv.history(), st3["alpha_p"], st3["alpha_d"])
        assert len(one_launch[1]) == 3

        sv.set_state(*case.state())
        errs = {}
        for k in range(3):
            x, y, s = (v.ravel().copy() for v in sv.get_state())
            wz = sv.get_bound_state()
            w, z = (v.ravel().copy() for v in wz) if wz is not None else (case.w, case.z)
            o = Q.iterate(case.copy(x=x, y=y, s=s, w=w, z=z), g)
            st = sv.iterate(1)
            hist = sv.history()
            assert len(hist) == k + 1 and hist[k]["k"] == k
            assert st["alpha_p"] == st["alpha_d"] and hist[k]["alpha_aff_p"] == hist[k]["alpha_aff_d"]
            xn, yn, sn = sv.get_state()
            got = {"x": xn, "s": sn, "y": yn, "ATy": case.A.T @ yn.ravel(), "alpha_p": st["alpha_p"], "alpha_d": st["alpha_d"]}
            if case.bounded:
                got["w"], got["z"] = sv.get_bound_state()
            got.update({"hist." + q: hist[k][q] for q in HIST_SCALARS})
            for q, v in got.items():
                errs.update({"step%d.%s" % (k, q2): e for q2, e in measure(q, v, o).items()})
        three_launches = (_bits(sv), sv.history(), st["alpha_p"], st["alpha_d"])
    assert three_launches[1] == one_launch[1], name                       # the three records, bit for bit: they are doubles
    assert three_launches[0] == one_launch[0] and three_launches[2:] == one_launch[2:], name
    _assert_all(name, errs, {q: _bound(q) for q in errs})


# ---- 3. whole solves --------------------------------------------------------------------------------------------------------
def _solve(name, flagged=True, after=None, quad="problem", **kw):
    """A fresh CSC handle on that problem, solved from the reference start -> what check_solve reads, plus _collect's record."""
    A, b, c, g, u, xs, ys = QS.problem(name)
    quad = g if isinstance(quad, str) else quad
    make = _small if flagged else (lambda A, b, c, **k: ipm.IpmSolver(sparse.csc_matrix(A), b, c, **k))
    with make(A, b, c, ub=u, quad=quad, **kw) as sv:
        if after:
            after(sv)
        sv.init_state(1.0)
        st = sv.solve(tol=Q.TOL)
        x, y, s = (v.ravel() for v in sv.get_state())
        wz = sv.get_bound_state()
        return dict(st=st, x=x, y=y, s=s, w=None if wz is None else wz[0].ravel(), z=None if wz is None else wz[1].ravel(),
                    hist=sv.history(), schedule=sv.schedule(), nonzeros=sv.quadratic_nonzeros(), record=_collect(sv))


@pytest.mark.parametrize("name", sorted(QS.SOLVES))
def test_whole_solve(name):
    r = _solve(name)
    assert r["schedule"]["fused_small"] == 1 and r["nonzeros"] > 0
    with QS.solves_registered():
        check_solve(name, name, r)


def test_whole_solve_agrees_with_the_multi_kernel_path():
    name = "small/50x130bm"
    small, multi = _solve(name), _solve(name, flagged=False)
    assert small["schedule"]["fused_small"] == 1 and multi["schedule"]["fused_small"] == 0
    assert small["st"]["status"] == multi["st"]["status"] == 1
    assert abs(small["st"]["iterations"] - multi["st"]["iterations"]) <= 2
    assert abs(small["st"]["objective"] - multi["st"]["objective"]) <= 1e-9 * abs(multi["st"]["objective"])
    print("OBS iterations small %d multi-kernel %d, device ms small %.3f multi-kernel %.3f"
          % (small["st"]["iterations"], multi["st"]["iterations"], small["st"]["solve_ms"], multi["st"]["solve_ms"]))


def test_front_end_reports_the_path():
    A, b, c, g, u, xs, ys = QS.problem("small/50x130bm")
    A = sparse.csc_matrix(A)
    x, y, s, info = ipm.solve_with_info(A, b, c, ub=u, quad=g, quad_small=True, tol=Q.TOL)
    assert info["status"] == 1 and info["quadratic"] == int((g > 0).sum()) and info["quadratic_path"] == "small"
    assert np.linalg.norm(x.ravel() - xs) / np.linalg.norm(xs) <= max(1e-9, 100 * QS.host_loop("small/50x130bm")["x_err"])
    assert ipm.solve_with_info(A, b, c, ub=u, quad=g, tol=Q.TOL, max_iter=3)[3]["quadratic_path"] == "multi-kernel"      # the default
    assert ipm.solve_with_info(A, b, c, ub=u, quad_small=True, tol=Q.TOL, max_iter=3)[3]["quadratic_path"] is None
    x2 = ipm.solve(A, b, c, ub=u, quad=g, quad_small=True, tol=Q.TOL)[0]
    assert np.array_equal(x2, x)


# ---- 4. invariants ----------------------------------------------------------------------------------------------------------
INVARIANT = "small/50x130bm"


def test_bitwise_repeat():
    a, b = _solve(INVARIANT), _solve(INVARIANT)
    assert a["st"]["status"] == 1 and a["record"] == b["record"]


def test_the_flag_alone_changes_nothing():
    """A flagged handle with no term, and one whose term was set and cleared (NULL, all zeros), run the LP variant: the unflagged LP
    handle's state, history and statistics, bit for bit."""
    A, b, c, g, u, xs, ys = QS.problem(INVARIANT)
    n = c.shape[0]

    def run(flagged, quad, after=None):
        make = _small if flagged else (lambda A, b, c, **k: ipm.IpmSolver(sparse.csc_matrix(A), b, c, **k))
        with make(A, b, c, ub=u, quad=quad) as sv:
            assert sv.schedule()["fused_small"] == 1
            if after:
                after(sv)
            assert sv.quadratic_nonzeros() == 0
            sv.init_state(1.0)
            sv.solve(tol=Q.TOL, max_iter=9)
            return _collect(sv)
    lp = run(False, None)
    assert len(lp[1]) > 0
    assert run(True, None) == lp
    assert run(True, g, after=lambda sv: sv.set_quadratic(None)) == lp
    assert run(True, g, after=lambda sv: sv.set_quadratic(np.zeros(n))) == lp
    with _small(A, b, c, ub=u, quad=g) as sv:                             # (and the term does change the trajectory)
        sv.init_state(1.0)
        sv.solve(tol=Q.TOL, max_iter=9)
        assert _collect(sv)[1] != lp[1]


def test_independent_of_check_every():
    a, b = _solve(INVARIANT, check_every=1), _solve(INVARIANT, check_every=7)
    assert a["st"]["status"] == 1 and a["record"] == b["record"]


def test_term_before_or_after_A():
    A, b, c, g, u, xs, ys = QS.problem(INVARIANT)
    before = _solve(INVARIANT)
    after = _solve(INVARIANT, quad=None, after=lambda sv: sv.set_quadratic(g))
    assert after["nonzeros"] == before["nonzeros"] == int((g > 0).sum())
    assert before["st"]["status"] == 1 and before["record"] == after["record"]


@pytest.mark.parametrize("order", ["before", "after"])
def test_equilibration_equals_the_prescaled_problem(order):
    """The rule of tests/test_gpu_equilibrate.py on the small path: scale="ruiz" given g is bit-identical, after unscaling, to an
    unscaled handle given the host-prescaled (R A C, R b, C c, u / C, g C^2): ipm_equilibrate rescales g AND the product list."""
    A, b, c, g, u, xs, ys = QS.problem(INVARIANT)
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
        with _small(*args, ub=ub, scale="ruiz" if scaled else None, quad=gg if (order == "before" or not scaled) else None) as sv:
            if scaled:
                assert np.array_equal(sv.scaling()[1], Cc) and sv.scale_info["passes"] == changed
                if order == "after":
                    sv.set_quadratic(gg)
            assert np.array_equal(sv.quadratic(), gg) and sv.schedule()["fused_small"] == 1
            sv.init_state(1.0)
            st = sv.solve(tol=Q.TOL, max_iter=40)
            out.append((st, sv.history(), sv.get_state(), sv.get_bound_state()))
    (st1, h1, (x1, y1, s1), wz1), (st2, h2, (x2, y2, s2), wz2) = out
    for k in st1:
        if k != "solve_ms":
            assert st1[k] == st2[k], (k, st1[k], st2[k])
    assert st1["iterations"] > 0 and h1 == h2
    Rc, Cv = R.reshape(-1, 1), Cc.reshape(-1, 1)
    assert np.array_equal(x1, Cv * x2) and np.array_equal(y1, Rc * y2) and np.array_equal(s1, s2 / Cv)
    assert np.array_equal(wz1[0], Cv * wz2[0]) and np.array_equal(wz1[1], wz2[1] / Cv)


# ---- 5. batch ---------------------------------------------------------------------------------------------------------------
def _make(P):
    sv = _small(P["A"], P["b"], P["c"], ub=P["ub"], quad=P.get("quad"), detect_infeasibility=P["detect"])
    return sv


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


def test_all_six_variants_in_one_call():
    """Two handles of every kernel variant in a shuffled order; one of the QPs has more than 5 % duplicated rows, so the second,
    shifted round of the call runs a quad variant.  Nothing is compared approximately."""
    Ps = [synthetic(30, 80, seed=1), synthetic(100, 240, seed=2)]                                                  # plain
    Ps += [_with_bounds(synthetic(40, 100, seed=s), s) for s in (3, 4)]                                            # bounded
    Ps += [dict(synthetic(36, 90, seed=s), detect=True) for s in (5, 6)]                                           # detect
    Ps += [dict(_with_bounds(synthetic(40, 100, seed=s), s), detect=True) for s in (7, 8)]                         # bounded + detect
    dup = _with_term(duplicated_rows_lp(), 9)
    Ps += [_with_term(synthetic(50, 130, seed=10), 10), dup]                                                       # quad
    Ps += [_with_term(_with_bounds(synthetic(40, 100, seed=s), s), s) for s in (11, 12)]                           # bounded + quad
    variant = lambda P: (P["ub"] is not None, bool(P["detect"]), P.get("quad") is not None)          # noqa: E731
    assert sorted(variant(P) for P in Ps) == sorted(2 * [(bd, dt, qd) for bd in (False, True) for dt, qd in ((False, False), (True, False), (False, True))])
    order = np.random.default_rng(7).permutation(len(Ps))
    assert not np.array_equal(order, np.arange(len(Ps)))
    Ps = [Ps[i] for i in order]
    refs = [_solo(P) for P in Ps]
    got = _batch(Ps)
    for P, g, r in zip(Ps, got, refs):
        assert_same(g, r, P["name"])
    shifted = {P["name"]: g["stats"]["auto_regularized"] for P, g in zip(Ps, got)}
    assert shifted[dup["name"]] == 1 and sum(shifted.values()) == 1, shifted
    assert all(g["stats"]["alpha_p"] == g["stats"]["alpha_d"] for P, g in zip(Ps, got) if P.get("quad") is not None)
    assert sum(g["stats"]["status"] == 1 for g in got) >= 10, [g["stats"]["status"] for g in got]


def test_300_qps_equal_solo():
    """300 distinct 17 x 40 QPs in one call: more workgroups than the 256 compute units.  ALL are compared bit for bit."""
    Ps = [_with_term(synthetic(17, 40, seed=20_000 + k), k) for k in range(300)]
    refs = [_solo(P, max_iter=100) for P in Ps]
    got = _batch(Ps, max_iter=100)
    for P, g, r in zip(Ps, got, refs):
        assert_same(g, r, P["name"])
    assert sum(g["stats"]["status"] == 1 for g in got) >= 150


def test_python_front_end_equals_solve_with_info():
    problems, ub = [], []
    for name in ("small/17x40b", "small/16x40m", "small/50x130bm"):
        A, b, c, g, u, xs, ys = QS.problem(name)
        problems += [(sparse.csc_matrix(A), b, c, g), (A, b, c, None), (A, b, c, np.zeros(A.shape[1]))]      # the QP, and its LP twice
        ub += [u, u, u]
    got = ipm.solve_small_qp_batch(problems, tol=Q.TOL, ub=ub, max_iter=60)
    assert len(got) == len(problems)
    skip = ("solve_ms", "setup_seconds", "solve_seconds", "teardown_seconds")
    for i, ((A, b, c, g), u, (x, y, s, info)) in enumerate(zip(problems, ub, got)):
        xr, yr, sr, ref = ipm.solve_with_info(sparse.csc_matrix(A), b, c, ub=u, quad=g, quad_small=True, tol=Q.TOL, max_iter=60)
        assert np.array_equal(x, xr) and np.array_equal(y, yr) and np.array_equal(s, sr), i
        assert set(info) == set(ref) - {"setup_seconds", "solve_seconds", "teardown_seconds"}, i
        for k, v in info.items():
            if k in skip:
                continue
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, ref[k]), (i, k)
            else:
                assert v == ref[k] or (v != v and ref[k] != ref[k]), (i, k, v, ref[k])
        want = int((g > 0).sum()) if g is not None else 0
        assert info["quadratic"] == want and info["quadratic_path"] == ("small" if want else None)
    assert got[0][3]["status"] == 1 and got[0][3]["objective"] != got[1][3]["objective"]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _small_problem():
    A, b, c, g, u, xs, ys = workloads.separable_qp(50, 130, 5)
    return sparse.csc_matrix(A), b, c, g


def test_without_the_flag_both_orders_behave_as_before():
    A, b, c, g = _small_problem()
    with ipm.IpmSolver(A, b, c) as sv:                                     # A first: the one-workgroup path is taken ...
        assert sv.schedule()["fused_small"] == 1 and not sv.quad_small
        with pytest.raises(ipm.IpmError, match="before A") as ei:          # ... and a term then is refused
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
        sv.set_quadratic(None)                                             # clearing is always accepted
        sv.set_quadratic(np.zeros(sv.n))
        sv.init_state(1.0)
        assert sv.solve(tol=Q.TOL, max_iter=3)["iterations"] > 0           # and the handle stays usable
    with ipm.IpmSolver(A, b, c, quad=g) as sv:                             # the term first: never the small path
        assert sv.schedule()["fused_small"] == 0 and sv.quadratic_nonzeros() == int((g > 0).sum())
    with ipm.IpmSolver(A, b, c, quad=g, quad_small=False) as sv:
        assert sv.schedule()["fused_small"] == 0


def test_the_flag_has_no_effect_beyond_the_small_path():
    A, b, c, g, u, xs, ys = Q.problem("200x520b")                          # 200 rows: does not qualify
    out = []
    for flag in (False, True):
        with ipm.IpmSolver(sparse.csc_matrix(A), b, c, ub=u, quad=g, quad_small=flag, factor="dense") as sv:
            assert sv.schedule()["fused_small"] == 0
            sv.init_state(1.0)
            sv.solve(tol=Q.TOL, max_iter=6)
            out.append(_collect(sv))
    assert out[0] == out[1]


def test_with_the_flag_every_refusal_stays():
    A, b, c, g = _small_problem()
    with pytest.raises(ValueError, match="detect_infeasibility"):         # the host's refusal, before a handle exists
        ipm.IpmSolver(A, b, c, quad=g, quad_small=True, detect_infeasibility=True)
    with _small(A, b, c, detect_infeasibility=True) as sv:                 # the library's own
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_DETECT_INFEASIBILITY") as ei:
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
    with pytest.raises(ValueError, match="lockstep"):
        ipm.IpmSolver(A, b, c, quad=g, quad_small=True, lockstep=True)
    with ipm.IpmSolver(A, b, c, quad_small=True, lockstep=True) as sv:
        with pytest.raises(ipm.IpmError, match="IPM_FLAG_LOCKSTEP") as ei:
            sv.set_quadratic(g)
        assert ei.value.code == -1 and sv.quadratic_nonzeros() == 0
    with _small(A, b, c, quad=g) as sv:
        with pytest.raises(ipm.IpmError, match="quadratic term") as ei:    # correctors: the term's reason comes first
            sv.set_correctors(1)
        assert ei.value.code == -1 and sv.correctors == 0
        with pytest.raises(ipm.IpmError, match="fused small-LP kernel") as ei:
            sv.set_refine(1)
        assert ei.value.code == -1 and sv.refine == 0
        sv.set_quadratic(None)
        with pytest.raises(ipm.IpmError, match="fused small-LP kernel"):   # and without the term, the path's
            sv.set_correctors(1)
        sv.init_state(1.0)
        assert sv.solve(tol=Q.TOL, max_iter=3)["iterations"] > 0           # the handle stays usable
    with pytest.raises(ValueError, match="correctors"):
        ipm.IpmSolver(A, b, c, quad=g, quad_small=True, correctors=1)
    with pytest.raises(ipm.IpmError, match="fused small-LP kernel"):
        ipm.IpmSolver(A, b, c, quad=g, quad_small=True, refine=1)
    with pytest.raises(ValueError, match="dense_cols needs a sparse A of more than 128 rows"):
        ipm.IpmSolver(A, b, c, quad=g, quad_small=True, dense_cols=[0])
    svs = [_small(A, b, c, quad=g)]
    try:
        svs[0].init_state(1.0)
        for kw in (dict(correctors=1), dict(refine=1), dict(dense_cols=[0])):
            with pytest.raises(ValueError):
                ipm.solve_small_batch_solvers(svs, **kw)
    finally:
        svs[0].close()
