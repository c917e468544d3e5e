"""One interior-point iteration on the device at NEAR-OPTIMAL states, against the longdouble oracle of tests/iteration_oracle.py.

Every other comparison of an iteration with a reference starts from a benign interior point (x, s, w, z ~ U(0.5, 2), theta in
[0.25, 4]).  The last iterations of a solve run elsewhere: theta spans 1/mu .. mu over a basic / non-basic partition, A Theta A^T is
formed from terms 16 orders of magnitude apart, dx = theta (A^T dy) + theta t cancels to eps / mu, ds divides by mu-sized numbers,
every ratio test has n near-blockers, sigma sits near 0.  There the suite checked only that whole solves converge, which forgives
a direction that is three digits worse than it should be.  tests/late_cases.py builds such states (nondeg |B| = m, dualdeg
|B| = m + 20, primdeg |B| = m - 10; mu = 1e-3 .. 1e-8); tests/test_late_cases_host.py asserts, without a GPU, that they are what they
claim and that the bounds below mean something.

The sequence per cell is test_gpu_iteration_edges.check_iteration's (both directions, iterate(1), the history record), with
  * the measures of late_cases.measure: 2-norm relative error of vectors; the next x, s, w, z also componentwise ("x.cw": the 2-norm
    cannot see their mu-sized half); sigma by its absolute error; every other scalar as check_iteration measures it;
  * the bound of a cell: max(floor(quantity), MARGIN x H(case, quantity)), H the error of the float64 HOST restatement against the
    same oracle, maximum over three column orders; MARGIN = 16.  No bound comes from the device.  A cell whose three host orders
    spread by more than STABLE = 4 is dropped (printed, not asserted): 20 of 896 cells, 2.2 %, see the host file.

Cells (the smallest shapes that reach each path, asserted through schedule() / factor_info()):
    dense 130 x 257, the eight family / mu points, plain and bounded      2 blocks, one 256-row group inverse; the vector kernels
    dense 300 x 513 bounded, dualdeg 1e-8 and primdeg 1e-3                3 blocks: no group, the block-step substitutions
    dense 129 x 16385 bounded, dualdeg 1e-8                               the grid-stride trip, two-level reductions over 16 orders
    dense 1000 x 2000, primdeg 1e-3 plain and dualdeg 1e-8 bounded        8 blocks: one 1024-row group inverse (refinement oracle)
    CSC 130 x 300 bounded dualdeg 1e-6, factor dense and sparse           envelope factor; multifrontal factor and its sweeps
    CSC 60 x 150 bounded dualdeg 1e-6, IPM_FUSED_SMALL 1 and 0            the one-workgroup path's copy of the rules, and its twin
    two lockstep handles (257 x 520 dualdeg 1e-8, 130 x 300 primdeg 1e-3) solve_lockstep(max_iter=1): the batched twins, block steps (3 blocks) and grouped
    QP 130 x 257 bounded dualdeg 1e-6, against qp_oracle                  the Quad rules at theta = 1 / (s/x + z/w + g), s/x ~ mu
Exact assertions in every cell: the next iterate strictly positive and finite, pivots_fixed == 0 (the oracle has no guard); one
cell repeated bit for bit; the QP cell's alpha_p == alpha_d.

The stop decision at a late state: three states whose binding inequality is rp, rd and the gap in turn (tau = the smallest tolerance
at which the oracle says converged): solve(tol = 2 tau) returns CONVERGED after 0 iterations with the state untouched bit for bit,
solve(tol = tau / 2, max_iter = 3) takes at least one iteration.  On the multi-kernel path (dense 130 x 257) and on the
one-workgroup path, which serves CSC matrices of at most 128 rows (60 x 150).

Observed on MI355X (first run of this file; every cell passed, so nothing below is a bound): per quantity, the largest device error
over max(H, floor / MARGIN) -- a cell passes while this is <= MARGIN = 16 -- and the cell that gave it (OBSERVED_LATE below).
    sigma 7.2 (lockstep 257 x 520 dualdeg 1e-8); alpha_aff_p 6.8, alpha_p 6.7 (130 x 257 dualdeg 1e-6); alpha_d 4.4 (300 x 513 dualdeg
    1e-8); alpha_aff_d 3.9 (130 x 257 bounded primdeg 1e-4): the step lengths, whose ratio tests have n near-blockers
    every direction (dxa .. dz, A^T dy) 1.8 .. 3.1 and the next x 2.7: 130 x 257 nondeg 1e-4 bounded, primdeg 1e-4 and the QP cell
    componentwise x 2.3, z 2.3, w 1.5, s 1.4; next s, y, w, z, A^T y 1.2 .. 1.4; residual norms, objective, mu, gap below 0.07
The device loses nowhere an order of magnitude more than float64 on the host does; 16 of its 943 cells are dropped ones.

What the file can and cannot see, tried with deliberately wrong rules in scratch builds of the library (none committed):
  * x * (1.0 / s) for x / s (vector_ops.h, quad_theta) and r4 / w - z r_u / w for (r4 - z r_u) / w (the bounded t): one-ulp changes of
    one factor.  Every cell stayed green and the largest ratio stayed 7.2: such a change is below what float64 itself loses here, so
    a bound of MARGIN x H cannot flag it, here or on the host.
  * x / (s + 1e-14), a "safe division" (vector_ops.h, bnd_theta, small_lp.h): a relative error of 1e-14 in theta at the benign states,
    1e-6 at s ~ 1e-8.  11 of the 34 tests of this file turn red (every dualdeg cell of mu <= 1e-6, both sparse factors, the small
    path and its twin, the lockstep pair: step lengths and sigma up to 280 x H, dw and componentwise w near 60 x H) while all of
    test_gpu_iteration_edges.py and test_gpu_qp.py stay green.
"""
import numpy as np
import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

import late_cases as LC
from test_gpu_iteration_edges import _assert_all, _solver, check_iteration

pytestmark = pytest.mark.gpu

# per quantity: (the largest device error / max(H, floor / MARGIN) over all cells -- a cell passes while this is <= MARGIN --, the cell)
OBSERVED_LATE = {"ATdy": (2.8, "qp/130x257b/dualdeg/1e-06"), "ATdya": (2.9, "dense/130x257b/nondeg/1e-04"), "ATy": (1.3, "dense/130x257b/primdeg/1e-04"),
                 "alpha_aff_d": (3.9, "dense/130x257b/primdeg/1e-04"), "alpha_aff_p": (6.8, "dense/130x257/dualdeg/1e-06"),
                 "alpha_d": (4.4, "dense/300x513b/dualdeg/1e-08"), "alpha_p": (6.7, "dense/130x257b/dualdeg/1e-06"), "ds": (2.8, "qp/130x257b/dualdeg/1e-06"),
                 "dsa": (3.1, "dense/130x257b/nondeg/1e-04"), "dw": (1.8, "qp/130x257b/dualdeg/1e-06"), "dx": (2.8, "dense/130x257/primdeg/1e-04"),
                 "dxa": (2.8, "dense/130x257/primdeg/1e-04"), "dy": (2.7, "dense/130x257b/nondeg/1e-04"), "dya": (3.0, "dense/130x257b/nondeg/1e-04"),
                 "dz": (3.1, "qp/130x257b/dualdeg/1e-06"), "gap": (0.002, "dense/130x257/nondeg/1e-04"), "mu": (0.003, "sparse/60x150b/dualdeg/1e-06/fused_small=1"),
                 "objective": (0.029, "dense/130x257b/primdeg/1e-03"), "rd_norm": (0.049, "dense/130x257b/nondeg/1e-08"),
                 "rp_norm": (0.063, "dense/129x16385b/dualdeg/1e-08"), "s": (1.3, "dense/130x257b/primdeg/1e-04"), "s.cw": (1.4, "dense/129x16385b/dualdeg/1e-08"),
                 "sigma": (7.2, "lock/257x520/dualdeg/1e-08"), "w": (1.2, "dense/129x16385b/dualdeg/1e-08"), "w.cw": (1.5, "dense/130x257b/dualdeg/1e-06"),
                 "x": (2.7, "dense/130x257/primdeg/1e-04"), "x.cw": (2.3, "dense/130x257b/dualdeg/1e-08"), "y": (1.4, "dense/130x257b/primdeg/1e-04"),
                 "z": (1.2, "dense/130x257b/primdeg/1e-04"), "z.cw": (2.3, "dense/130x257b/primdeg/1e-04")}


def _recorder(name):
    """late_cases.measure, keeping what it returned: -> (measure, seen)."""
    seen = {}

    def measure(quantity, got, o):
        e = LC.measure(quantity, got, o)
        seen.update(e)
        return e
    return measure, seen


def _report(cell, name, seen, ev=None):
    ev = ev or LC.evaluate(name)
    for k in sorted(seen):
        print("LATE %s %s error %.3e H %.3e floor %.1e over %.3f%s" % (cell, k, seen[k], ev.H[k], LC.floor(k),
              seen[k] / max(ev.H[k], LC.floor(k) / LC.MARGIN), " DROPPED (host spread %.1f)" % ev.spread[k] if k in ev.dropped else ""))


def _exact(cell, sv, case, st, h):
    x, y, s = (v.ravel() for v in sv.get_state())
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(s)) and np.all(x > 0) and np.all(s > 0), cell
    if case.bounded:
        w, z = (v.ravel() for v in sv.get_bound_state())
        U = case.U
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(z)) and np.all(w[U] > 0) and np.all(z[U] > 0), cell
    assert st["pivots_fixed"] == 0 and h["pivots_fixed"] == 0, (cell, st["pivots_fixed"], h["pivots_fixed"])


def check_late(cell, name, sv, ev=None):
    """ev: the evaluated case where it is not one of late_cases.CASES (tests/test_gpu_late_large.py)."""
    ev = ev or LC.evaluate(name)
    measure, seen = _recorder(name)
    try:
        o, st, h = check_iteration(cell, sv, ev.case, o=ev.o, measure=measure, bound=LC.bound_of(ev))
    finally:
        _report(cell, name, seen, ev)
    _exact(cell, sv, ev.case, st, h)
    return st, h


def _assert_dense(sv, case, blocks, grouped=1):
    """grouped: 1 the group inverses + GEMV substitutions of trsv_grouped.h (the blocks divide into groups of 2, 4 or 8), 0 block steps."""
    sch = sv.schedule()
    assert not sv.sparse and sv.factor == "dense" and sch["fused_small"] == 0 and sch["blocks"] == blocks == (case.m + 127) // 128, sch
    assert sch["grouped_trsv"] == grouped, sch
    assert (sv.m, sv.n) == (case.m, case.n) and sv.bounded == int(case.U.sum())


# ---- dense ingest ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.D130)
def test_dense_130x257(name):
    case = LC.get(name)
    with _solver(case) as sv:
        _assert_dense(sv, case, 2)
        check_late(name, name, sv)


@pytest.mark.parametrize("name", LC.D300)
def test_dense_300x513(name):
    case = LC.get(name)
    with _solver(case) as sv:
        _assert_dense(sv, case, 3, grouped=0)                  # three blocks form no group: the block-step substitutions
        check_late(name, name, sv)


def test_dense_129x16385_past_the_stride():
    case = LC.get(LC.D129)
    assert int((case.part == LC.BASIC).sum()) == 149
    with _solver(case) as sv:
        _assert_dense(sv, case, 2)
        check_late(LC.D129, LC.D129, sv)


@pytest.mark.parametrize("name", LC.D1000)
def test_dense_1000x2000_one_1024_row_group(name):
    case = LC.get(name)
    with _solver(case) as sv:
        _assert_dense(sv, case, 8)
        check_late(name, name, sv)


def test_bitwise_repeat():
    name = LC.name_of("dense", 130, 257, True, "dualdeg", 1e-8)
    case = LC.get(name)
    runs = []
    for _ in range(2):
        with _solver(case) as sv:
            sv.set_state(*case.state())
            st = sv.iterate(1)
            runs.append(([v.tobytes() for v in sv.get_state() + sv.get_bound_state()], sv.history(), st["alpha_p"], st["alpha_d"]))
    assert runs[0] == runs[1]


# ---- sparse ingest ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", ["dense", "sparse"])
def test_sparse_ingest(factor):
    case = LC.get(LC.S130)
    with _solver(case, as_sparse=True, factor=factor) as sv:
        sch = sv.schedule()
        assert sv.sparse and sv.factor == factor and sch["fused_small"] == 0 and sv.bounded == int(case.U.sum())
        if factor == "dense":
            assert sch["blocks"] == 2, sch
        else:
            assert sv.factor_info()["panels"] >= 1
        check_late("%s/factor=%s" % (LC.S130, factor), LC.S130, sv)


@pytest.mark.parametrize("fused", [1, 0])
def test_small_path_and_its_multi_kernel_twin(fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("IPM_FUSED_SMALL", "0")
    case = LC.get(LC.S60)
    with _solver(case, as_sparse=True) as sv:
        sch = sv.schedule()
        assert sv.sparse and sch["fused_small"] == fused and sv.factor == "dense" and sv.bounded == 75, sch
        check_late("%s/fused_small=%d" % (LC.S60, fused), LC.S60, sv)


# ---- lockstep twins --------------------------------------------------------------------------------------------------------
def check_lockstep(names, evaluate, group_blocks):
    """solve_lockstep(max_iter=1) of the named cases as one batch, every LP against its oracle.  evaluate: name -> the evaluated case;
    group_blocks: per case, what schedule() must report (0: block steps)."""
    evs = [evaluate(nm) for nm in names]
    cases = [ev.case for ev in evs]
    svs = [_solver(case, as_sparse=True, lockstep=True, factor="dense") for case in cases]
    try:
        for sv, case, gb in zip(svs, cases, group_blocks):
            sch = sv.schedule()
            assert ipm.lockstep_eligible(sv) and sch["fused_small"] == 0 and sv.factor == "dense" and not sv.bounded
            assert sch["blocks"] == (case.m + 127) // 128 and sch["grouped_trsv"] == (1 if gb else 0) and sch["group_blocks"] == gb, sch
            sv.set_state(*case.state())
        stats = ipm.solve_lockstep(svs, tol=1e-30, max_iter=1)
        for name, sv, ev, st in zip(names, svs, evs, stats):
            case = ev.case
            assert st["iterations"] == 1 and st["status"] == _lib.STATUS_MAX_ITER, (name, st)
            hist = sv.history()
            assert len(hist) == 1 and hist[0]["k"] == 0
            h = hist[0]
            assert h["alpha_p"] == st["alpha_p"] and h["alpha_d"] == st["alpha_d"]
            x, y, s = sv.get_state()
            got = {"x": x, "s": s, "ATy": case.A.T @ y.ravel(), "y": y, "alpha_p": st["alpha_p"], "alpha_d": st["alpha_d"]}
            got.update({"hist." + k: h[k] for k in LC.HIST_SCALARS})
            e = {}
            for q, v in got.items():
                e.update(LC.measure(q, v, ev.o))
            _report(name, name, e, ev)
            bound = LC.bound_of(ev)
            _assert_all(name, e, {k: bound(k) for k in e})
            _exact(name, sv, case, st, h)
            assert sv.schedule()["timeouts_recovered"] == 0
    finally:
        for sv in svs:
            sv.close()


def test_lockstep_pair():
    check_lockstep(LC.LOCK, LC.evaluate, [0, 2])                # 257 rows: 3 blocks, block steps; 130 rows: one 256-row group


# ---- the QP ----------------------------------------------------------------------------------------------------------------
def test_qp():
    ev = LC.evaluate(LC.QP)
    case, g = ev.case, ev.g
    assert int((g > 0).sum()) == (case.n + 1) // 2
    with ipm.IpmSolver(case.A, case.b, case.c, ub=case.ub(), quad=g) as sv:
        _assert_dense(sv, case, 2)
        assert np.array_equal(sv.quadratic(), g) and sv.quadratic_nonzeros() == int((g > 0).sum())
        st, h = check_late(LC.QP, LC.QP, sv)
        assert st["alpha_p"] == st["alpha_d"] and h["alpha_aff_p"] == h["alpha_aff_d"]           # ONE step length, exactly


# ---- the stop decision -----------------------------------------------------------------------------------------------------
def _bits(sv):
    return [v.tobytes() for v in sv.get_state() + sv.get_bound_state()]


@pytest.mark.parametrize("binding", sorted(LC.STOP_SCALES))
@pytest.mark.parametrize("path", sorted(LC.STOP_SHAPES))
def test_stop_decision(path, binding):
    case = LC.stop_case(path, binding)
    tau = max(LC.stop_sides(case))
    with _solver(case, as_sparse=(path == "small")) as sv:
        assert sv.schedule()["fused_small"] == (1 if path == "small" else 0) and sv.bounded == int(case.U.sum())
        sv.set_state(*case.state())
        before = _bits(sv)
        st = sv.solve(tol=2 * tau)
        assert st["status"] == _lib.STATUS_CONVERGED and st["iterations"] == 0, (path, binding, st)
        assert _bits(sv) == before
        assert before == [np.ascontiguousarray(v, dtype=np.float64).tobytes() for v in (case.x, case.y, case.s, case.w, case.z)]
        sv.set_state(*case.state())
        st = sv.solve(tol=tau / 2, max_iter=3)
        assert st["iterations"] >= 1, (path, binding, st)
