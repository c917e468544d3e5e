"""The one-workgroup small-LP path (csrc/small_lp.h) against the longdouble oracle of tests/iteration_oracle.py, element by element, at
the edges of its own loops.  small_lp.h is the second, hand-kept implementation of the whole iteration: its own predictor column and
stop decision, the formation of A diag(d) A^T from a product list into LDS, potrf_lds on nt = ceil(m / 16) panels, both triangular
solves as 4-lane matvecs, every reduction, and y carried in LDS from one iteration to the next -- in four instantiations (plain,
bounded, detect, bounded + detect), each with a batch twin.  The suite held it to the oracle at 5 x 65 and 60 x 150 only; whole solves
converge through a slightly wrong direction, and batch == solo cannot see what both get wrong.

tests/small_path_cases.py builds the cells, tests/test_small_path_cases_host.py asserts without a GPU that they are what they claim
and that float64 alone meets the floor of the bounds on every one of them.  Every handle here is a CSC handle with
schedule()["fused_small"] asserted.

    test_one_iteration          every tile/, stride/, rows/ and list/ cell through test_gpu_iteration_edges.check_iteration: the next
                                x, s, y, w, z, the step lengths, sigma, mu, gap, objective and both residual norms of iterate(1) are
                                the small kernel's (newton_direction runs the multi-kernel kernels on the same handle)
    test_one_iteration_detect   the same on a detect handle, bounded and not (iterate runs under `force`: nothing fires)
    test_fire                   the small path's own sums and maxima of the infeasibility tests, the attaining column / row last
    test_fire_after_k_iterations  a test that fires first at the stop test of iteration K = 1, 2 or 3 of one launch: the running sums and
                                maxima of the tests after the resets between two stop tests (iterate() never evaluates them)
    test_carry_inside_one_launch  iterate(3) == three iterate(1) bit for bit, and every step of the trajectory against the oracle
                                started from the device state read back before it
    test_batch_twins_are_bitwise_the_solo_kernels   all four batch kernels in one call against solve() of a fresh handle
    test_late_128x300           a near-optimal state on eight tiles, with the measure and bound of tests/test_gpu_late_iteration.py
    test_list_limit             the rule terms <= 2^22 from both sides (128 x 508: 4 194 048 terms, 128 x 509: 4 202 304)

Bounds: test_gpu_iteration_edges._bound, max(1e-12, 100 x OBSERVED there), unchanged; the late cell max(floor, 16 H).

Observed maxima on MI355X (first run of this file; every test passed, so this is a record and not a bound), per quantity over the
cells of test_one_iteration, test_one_iteration_detect, test_carry_inside_one_launch and test_list_limit, and the cell that gave it
(OBSERVED_SMALL below).  What iterate(1) returns:
    x 4.1e-15, w 2.2e-15, sigma 9.5e-15, alpha_aff_d 1.0e-14 (list/full509, the multi-kernel side of the rule; the small kernel's
    largest: x 3.6e-15, w 2.1e-15 at list/full508, sigma 3.5e-15 at tile/17x40b, alpha_aff_d 1.2e-15 at tile/128x300b); s 4.0e-15, z 2.9e-15,
    dw 9.3e-15, dz 9.9e-15, alpha_d 5.3e-15, alpha_aff_p 8.9e-15 (list/full508); y 3.2e-15 (list/arrow); A^T y 2.8e-15 (tile/128x300b,
    second step of the carried trajectory); alpha_p 2.6e-15, rp_norm 1.2e-15 (stride/20x1025b, third step); mu, gap 2.8e-16, objective
    5.4e-16 (stride/20x513b); rd_norm 1.7e-16 (17 x 40 without bounds, detect)
The directions of newton_direction (the multi-kernel kernels on the same handles): dxa 1.5e-14, dx 1.0e-14, ds 9.8e-15, dsa 6.6e-15
(list/full509); dy 4.3e-15, dya 2.4e-15, A^T dy 2.3e-15, A^T dya 1.3e-15 (list/arrow).  The certificates of test_fire: normalization
3.7e-15, violation 3.6e-15 (primal, 20 x 513 bounded).  The late cell: at most 1.3 x max(H, floor / 16) (componentwise z), bound 16.

With deliberately wrong rules in scratch builds of the library (none committed; every one changes values only), of the 43 tests here:
  * the mirror store W[k*WLD+i] = acc dropped: 30 red (every one-iteration cell but 1 x 2, which has no off-diagonal entry, and
    list/full509, which is not on this path; the carry, late and limit tests; the primal delayed fire);
  * a 4-lane row sum of residual_rows started at pb + l4 + 4 for l4 == 3: 33 red (the same cells; the three dual-row cells of
    test_fire, whose ||A x||_inf is that sum; the delayed fire without bounds);
  * k < row4 for k <= row4 in the forward matvec: 32 red (with 1 x 2).
  Those three also turn test_small_path_and_its_multi_kernel_twin and the whole-solve tests of the small path red.
  * `ru2 = 0.0` removed: the six cells of test_carry_inside_one_launch red and nothing else -- every test of the small path the suite
    had before (both test_small_path_and_its_multi_kernel_twin, test_stop_decision, test_fused_small_lp_path, test_parity_small_lp_kb2,
    test_fused_small_lp, test_small_lp_guard, test_mixed_netlib_equals_solo) stays green.
  * `duz = 0.0; dmaty = 0.0; dmxu = 0.0` removed: test_fire_after_k_iterations red at its primal and its xu cell; `dmxu = 0.0` alone
    removed: red at its xu cell.  Nothing else turns red, here or among the 33 tests the suite had of the small path's detection,
    batches and residue (test_fused_small_lp, test_variants_in_one_call, test_small_path*, test_small_batch*, test_stop_decision).
  test_batch_twins_are_bitwise_the_solo_kernels stays green under all six, as it must: both sides are wrong together.
"""
import numpy as np
import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

import iteration_oracle as IO
import late_cases as LC
import small_path_cases as SP
from test_gpu_iteration_edges import DETECT, HIST_SCALARS, _assert_all, _bound, _check_certificate, _solver, check_iteration, measure
from test_gpu_late_iteration import _exact

pytestmark = pytest.mark.gpu

# per quantity: (the largest error of the first run on an MI355X, the cell); the bounds are test_gpu_iteration_edges._bound's
OBSERVED_SMALL = {"ATdy": (2.3e-15, "list/arrow"), "ATdya": (1.3e-15, "list/arrow"), "ATy": (2.8e-15, "tile/128x300b step 1"),
                  "alpha_aff_d": (1.0e-14, "list/full509"), "alpha_aff_p": (8.9e-15, "list/full508"), "alpha_d": (5.3e-15, "list/full508"),
                  "alpha_p": (2.6e-15, "stride/20x1025b step 2"), "ds": (9.8e-15, "list/full509"), "dsa": (6.6e-15, "list/full509"),
                  "dw": (9.3e-15, "list/full508"), "dx": (1.0e-14, "list/full509"), "dxa": (1.5e-14, "list/full509"), "dy": (4.3e-15, "list/arrow"),
                  "dya": (2.4e-15, "list/arrow"), "dz": (9.9e-15, "list/full508"), "gap": (2.8e-16, "stride/20x513b"), "mu": (2.7e-16, "stride/20x513b"),
                  "objective": (5.4e-16, "stride/20x513b"), "rd_norm": (1.7e-16, "detect/17x40"), "rp_norm": (1.2e-15, "stride/20x1025b step 2"),
                  "s": (4.0e-15, "list/full508"), "sigma": (9.5e-15, "list/full509"), "w": (2.2e-15, "list/full509"), "x": (4.1e-15, "list/full509"),
                  "y": (3.2e-15, "list/arrow"), "z": (2.9e-15, "list/full508")}


def _fused(name):
    return 0 if name == "list/full509" else 1


def _small(case, fused=1, **opts):
    """A CSC handle of the case, on the path the cell is there for."""
    sv = _solver(case, as_sparse=True, **opts)
    try:
        sch = sv.schedule()
        assert sv.sparse and sv.factor == "dense" and sch["fused_small"] == fused, sch
        assert (sv.m, sv.n) == (case.m, case.n) and sv.bounded == int(case.U.sum())
    except Exception:
        sv.close()
        raise
    return sv


def _bits(sv):
    return [v.tobytes() for v in sv.get_state() + (sv.get_bound_state() or ())]


# ---- one iteration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SP.BENIGN)
def test_one_iteration(name):
    case = SP.get(name)
    with _small(case, _fused(name)) as sv:
        o, st, h = check_iteration(name, sv, case)
        assert st["pivots_fixed"] == 0 and h["pivots_fixed"] == 0


@pytest.mark.parametrize("name", SP.DETECT_BENIGN)
def test_one_iteration_detect(name):
    """small_lp_detect_kernel and small_lp_bounded_detect_kernel: the rules of the iteration with the sums of the tests on the side."""
    case = SP.get(name)
    with _small(case, **DETECT) as sv:
        assert sv.detect_infeasibility
        o, st, h = check_iteration(name, sv, case)
        assert st["status"] not in (_lib.STATUS_PRIMAL_INFEASIBLE, _lib.STATUS_DUAL_INFEASIBLE) and sv.certificate() is None


@pytest.mark.parametrize("name", SP.FIRE)
def test_fire(name):
    """dby / duz / dmaty / dmax / dmxu of small_lp.h: beta, gamma and the violation of a known iterate.  The stop test skips detection
    under `force`, so the state is set and solve() called, not iterate()."""
    case = SP.get(name)
    with _small(case, **DETECT) as sv:
        sv.set_state(*case.state())
        st = sv.solve(tol=1e-8, max_iter=5)
        _check_certificate(name[len("detect/"):], sv, case, st)


@pytest.mark.parametrize("name", sorted(SP.DELAYED))
def test_fire_after_k_iterations(name):
    """A test that fires at the stop test of iteration K >= 1 of ONE launch (small_path_cases.delayed_fire chooses the tolerances
    from the oracle's trajectory): its normalization and violation against the oracle's quantities of the iterate at detection, which
    get_state returns.  duz, dmaty and dmxu are running sums and maxima: one the loop does not reset between two stop tests carries
    the earlier iterates into beta and the violations.  The iterate at detection is iterate(K)'s of the same handle, bit for bit."""
    d = SP.delayed_fire(name)
    case, K = d["case"], d["K"]
    with _small(case, detect_infeasibility=True, infeasibility_tol=d["tol"]) as sv:
        sv.set_state(*case.state())
        st = sv.solve(tol=1e-8, max_iter=5)
        x, y, s = (v.ravel().copy() for v in sv.get_state())
        w, z = (v.ravel().copy() for v in sv.get_bound_state()) if case.bounded else (case.w, case.z)
        at = case.copy(x=x, y=y, s=s, w=w, z=z)
        print("DELAYED %s K %d tol %s ratios %s at detection %s" % (name, K, d["tol"], d["ratios"], SP.fire_ratios(at)))
        _check_certificate("fire/%s/%s" % (d["kind"], name), sv, at, st, k=K)
        assert len(sv.history()) == K
        fired = _bits(sv)
        sv.set_state(*case.state())
        sv.iterate(K)
        assert _bits(sv) == fired, name


# ---- state carried across iterations inside one launch ---------------------------------------------------------------------
CARRY =["tile/17x40b", "tile/128x300b", "stride/20x1025b"]


@pytest.mark.parametrize("detect", [False, True], ids=["bounded", "bounded+detect"])
@pytest.mark.parametrize("name", CARRY)
def test_carry_inside_one_launch(name, detect):
    """(a) iterate(3) in one launch == three launches of iterate(1), bit for bit: a reset the loop misses (ru2, the detect sums, `red`)
    or a y that LDS carries differently from global memory breaks it.  (b) each of the three steps against the oracle started from
    the device state read back before the step: exact in float64, so no allowance for error growth."""
    case = SP.get(name)
    opts = DETECT if detect else {}
    cell = "%s/%s" % (name, "bounded+detect" if detect else "bounded")
    with _small(case, **opts) as sv:
        sv.set_state(*case.state())
        st3 = sv.iterate(3)
        assert st3["iterations"] == 3
        one_launch = (_bits(sv), sv.history(), st3["alpha_p"], st3["alpha_d"])
        assert len(one_launch[1]) == 3

        sv.set_state(*case.state())
        errs = {}
        for k in range(3):
            x, y, s = (v.ravel().copy() for v in sv.get_state())
            w, z = (v.ravel().copy() for v in sv.get_bound_state())
            at = case.copy(x=x, y=y, s=s, w=w, z=z)
            o = IO.iterate(at)
            st = sv.iterate(1)
            hist = sv.history()
            assert len(hist) == k + 1 and hist[k]["k"] == k
            xn, yn, sn = sv.get_state()
            wn, zn = sv.get_bound_state()
            got = {"x": xn, "s": sn, "y": yn, "ATy": case.A.T @ yn.ravel(), "w": wn, "z": zn, "alpha_p": st["alpha_p"], "alpha_d": st["alpha_d"]}
            got.update({"hist." + q: hist[k][q] for q in HIST_SCALARS})
            for q, v in got.items():
                errs.update({"step%d.%s" % (k, q2): e for q2, e in measure(q, v, o).items()})
        three_launches = (_bits(sv), sv.history(), st["alpha_p"], st["alpha_d"])
    assert three_launches[1] == one_launch[1], cell                       # the three records, bit for bit: they are doubles
    assert three_launches[0] == one_launch[0] and three_launches[2:] == one_launch[2:], cell
    _assert_all(cell, errs, {q: _bound(q) for q in errs})


# ---- the batch twins -------------------------------------------------------------------------------------------------------
def _collect(sv):
    stats = {k: v for k, v in sv.stats.items() if k != "solve_ms"}
    return _bits(sv), sv.history(), stats


def test_batch_twins_are_bitwise_the_solo_kernels():
    """One solve_small_batch_solvers call over every tile/, stride/ and rows/ cell and the benign detect/ cells: all four batch
    kernels.  Each handle against solve(max_iter=2) of a fresh handle from the same state.  (The detect handles keep the default
    tolerances here, so that no test fires and both iterations run.)"""
    names = [nm for nm in SP.BENIGN if not nm.startswith("list/")] + SP.DETECT_BENIGN
    opts = {nm: (dict(detect_infeasibility=True) if nm.startswith("detect/") else {}) for nm in names}
    variants = {(SP.get(nm).bounded, bool(opts[nm])) for nm in names}
    assert variants == {(False, False), (True, False), (False, True), (True, True)}
    solo = {}
    for nm in names:
        case = SP.get(nm)
        with _small(case, **opts[nm]) as sv:
            sv.set_state(*case.state())
            st = sv.solve(tol=1e-8, max_iter=2)
            assert st["iterations"] == 2 and st["status"] == _lib.STATUS_MAX_ITER, (nm, st)
            solo[nm] = _collect(sv)
    svs = []
    try:
        for nm in names:
            svs.append(_small(SP.get(nm), **opts[nm]))
            svs[-1].set_state(*SP.get(nm).state())
        stats = ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=2)
        for nm, sv, st in zip(names, svs, stats):
            assert st["iterations"] == 2 and st["status"] == _lib.STATUS_MAX_ITER, (nm, st)
            bits, hist, stats_ = _collect(sv)
            assert len(hist) == 2 and hist == solo[nm][1], nm
            assert bits == solo[nm][0], nm
            assert stats_ == solo[nm][2], (nm, stats_, solo[nm][2])
    finally:
        for sv in svs:
            sv.close()


# ---- a near-optimal state on eight tiles -----------------------------------------------------------------------------------
def test_late_128x300():
    ev = SP.late_evaluated()
    seen = {}

    def recording(quantity, got, o):
        e = LC.measure(quantity, got, o)
        seen.update(e)
        return e

    with _small(ev.case) as sv:
        try:
            o, st, h = check_iteration(SP.LATE_NAME, sv, ev.case, o=ev.o, measure=recording, bound=LC.bound_of(ev))
        finally:
            for k in sorted(seen):
                print("LATE %s %s error %.3e H %.3e floor %.1e over %.3f%s" % (
                    SP.LATE_NAME, k, seen[k], ev.H[k], LC.floor(k), seen[k] / max(ev.H[k], LC.floor(k) / LC.MARGIN),
                    " DROPPED (host spread %.1f)" % ev.spread[k] if k in ev.dropped else ""))
        _exact(SP.LATE_NAME, sv, ev.case, st, h)


# ---- the rule that decides whether a handle takes this path ----------------------------------------------------------------
def test_list_limit():
    """terms <= 2^22 (ipm_set_A_csc): 128 x 508 dense is the last product list that fits (4 194 048 terms), 128 x 509 the first that
    does not (4 202 304).  Each against its own oracle, on the path the rule gives it."""
    for name, fused in (("list/full508", 1), ("list/full509", 0)):
        case = SP.get(name)
        assert (SP.term_count(case.A) <= SP.TERM_LIMIT) == bool(fused)
        with _small(case, fused) as sv:
            assert sv.schedule()["fused_small"] == fused
            o, st, h = check_iteration("limit/" + name, sv, case)
            sv.set_state(*case.state())
            sv.newton_direction(False)
            dy = sv.newton_direction(True)[1]
            y = sv.get_state()[1]
            assert np.array_equal(y.ravel(), case.y)
            _assert_all("limit/" + name, {"dy": IO.rel(dy, o["dy"])}, {"dy": _bound("dy")})
