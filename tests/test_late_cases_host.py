"""The conditions under which tests/test_gpu_late_iteration.py means something, checked without a GPU (tests/late_cases.py has the
builders, the measures and the definitions of H, the spread and a dropped cell).

1. Every case is what its name claims: the partition sizes, max theta / min theta >= 1 / (16 mu^2) without bounds, every residual norm
   within [mu / 100, 100 mu sqrt(n)] of its data norm, no non-positive pivot in the oracle's Cholesky; cond(B) is printed.
2. H(case, quantity), the error of the float64 host restatement against the oracle in three column orders, is computed and printed
   with its spread, and the dropped cells stay inside three caps: at most 10 % of all cells; no case loses the 2-norm cells of x, s
   or y; every family keeps at least one case with all its cells.
3. The two oracle solves (direct longdouble formation; float64 Cholesky refined with longdouble residuals) agree on every LP case
   of m <= 300 to within 1/100 of the host error H of that cell, and every refinement ended stationary, including those of the
   1000 x 2000 cases, which have no direct oracle to compare with.
4. The floors of the new measures (componentwise x, s, w, z; sigma absolute) are 100 x the largest host error of that measure over
   the benign IO.ITER_CASES: recomputed here and compared with the constants late_cases.NEW_FLOORS.
5. The stop-test cases bind the inequality they are named after, with a factor 4 over the other two.

Observed on x86-64: 896 cells, 18 .. 21 dropped (2.0 .. 2.3 %) under 1, 4, 8 and 16 BLAS threads, nearly all of them step lengths of
primdeg cases, whose ratio tests have many near-blockers; every family kept 3 or more cases with all their cells.
"""
import numpy as np
import pytest

import iteration_oracle as IO
import late_cases as LC

NAMES = list(LC.CASES)
DROPPED_SHARE = 0.10


def _fmt(d):
    return " ".join("%s=%.1e" % (k, d[k]) for k in sorted(d))


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_claims(name):
    kind, shape, family, mu = name.split("/")
    mu = float(mu)
    case = LC.get(name)
    m, n = case.m, case.n
    assert IO.shape_name(m, n, case.bounded) == shape and case.mu_target == mu
    basic, lower, upper = (case.part == p for p in (LC.BASIC, LC.LOWER, LC.UPPER))
    assert int(basic.sum()) == m + LC.FAMILIES[family][0] and int(basic.sum() + lower.sum() + upper.sum()) == n
    U = case.U
    if case.bounded:
        assert int(U.sum()) == n // 2 and np.all(U[upper]) and 0 < int(upper.sum()) < int(U.sum())
        assert 0.2 < upper.sum() / (upper.sum() + (U & lower).sum()) < 0.6                    # "about 40 %" of the bounded at-lower columns
    else:
        assert not upper.any() and not case.w.any() and not case.z.any()
    big, small = (0.5, 2.0), (mu / 4, 4 * mu)

    def within(v, rng, on):
        return np.all((v[on] >= rng[0] * (1 - 1e-15)) & (v[on] <= rng[1] * (1 + 1e-15)))

    assert within(case.x, big, ~lower) and within(case.s, small, ~lower) and within(case.x, small, lower) and within(case.s, big, lower)
    assert within(case.w, small, upper) and within(case.z, big, upper) and within(case.w, big, U & ~upper) and within(case.z, small, U & ~upper)
    theta = case.x / case.s
    if not case.bounded:
        assert theta.max() / theta.min() >= 1 / (16 * mu * mu)
    if kind in ("sparse", "lock"):
        nz = case.A != 0
        assert nz.any(axis=0).all() and nz.any(axis=1).all() and nz.mean() < 0.15
    ev = LC.evaluate(name)                                                   # (a non-positive pivot of the oracle's Cholesky asserts there)
    o = ev.o
    LD = IO.LD
    rb = case.A.astype(LD) @ case.x.astype(LD) - case.b
    ru = np.where(U, case.x + case.w - np.where(U, case.u, 0.0), 0.0)
    rc = o["rd_norm"]
    for what, r, data in (("r_b", IO.norm(rb), IO.norm(case.b)), ("r_c", rc, o["c_norm"])) + \
            ((("r_u", IO.norm(ru), IO.norm(case.u[U])),) if case.bounded else ()):
        assert mu / 100 <= float(r / data) <= 100 * mu * np.sqrt(n), (name, what, float(r / data))
    assert float(o["mu"]) < 4 * mu and float(o["mu"]) > mu / 4
    print("CASE %s cond(B) %.2e (|B| = %d) theta %.1e .. %.1e mu %.2e" % (name, LC.basis_condition(case), basic.sum(), theta.min(),
                                                                          theta.max(), float(o["mu"])))


def test_host_error_is_computed_and_the_dropped_cells_stay_inside_the_caps():
    cells = dropped = 0
    complete = {f: [] for f in LC.FAMILIES}
    for name in NAMES:
        ev = LC.evaluate(name)
        assert len(ev.errs) == 3 and set(ev.H) == set(ev.errs[0]) and all(np.isfinite(v) for v in ev.H.values()), name
        cells += len(ev.H)
        dropped += len(ev.dropped)
        print("HOST %s\n  H      %s\n  spread %s\n  dropped %s" % (name, _fmt(ev.H), _fmt(ev.spread), sorted(ev.dropped)))
        for k in ev.dropped:
            assert ev.H[k] > LC.floor(k) and ev.spread[k] > LC.STABLE
        assert not ev.dropped & {"x", "s", "y"}, (name, ev.dropped)
        if not ev.dropped:
            complete[LC.FAMILY_OF[name]].append(name)
    print("DROPPED %d of %d cells: %.1f %%; cases with all their cells: %s" % (dropped, cells, 100.0 * dropped / cells,
                                                                               {f: len(v) for f, v in complete.items()}))
    assert dropped <= DROPPED_SHARE * cells
    assert all(complete.values()), complete


LP_SMALL = [nm for nm in NAMES if LC.get(nm).m <= 300 and not nm.startswith("qp/")]


@pytest.mark.parametrize("name", LP_SMALL)
def test_the_two_oracle_solves_agree(name):
    ev = LC.evaluate(name)
    assert ev.solver is None
    solver = LC.RefinementSolver()
    o2 = IO.iterate(ev.case.copy(), solver=solver)
    assert len(solver.log) == 2 and all(stationary for _, _, stationary in solver.log), solver.log
    e = LC.errors(ev.case, o2, ev.o)
    print("ORACLES %s rounds %s\n  %s" % (name, [r for r, _, _ in solver.log], _fmt(e)))
    bad = {k: (v, ev.H[k]) for k, v in e.items() if not v <= ev.H[k] / 100}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", LC.D1000)
def test_the_refinement_oracle_reached_stationarity(name):
    ev = LC.evaluate(name)
    assert ev.case.m > LC.REFINEMENT_ABOVE and ev.solver is not None
    assert len(ev.solver.log) == 2 and all(stationary for _, _, stationary in ev.solver.log), ev.solver.log
    print("REFINEMENT %s %s" % (name, ev.solver.log))


def test_floors_of_the_new_measures():
    """100 x the largest host error over the benign cases, against the pinned constants: equal within STABLE, the allowance for
    another summation order."""
    worst = {}
    for name in sorted(IO.ITER_CASES):
        case = IO.get(name)
        for k, v in LC.errors(case, LC.host_iteration(case), IO.iterate(case)).items():
            parts = k.split(".")
            key = parts[-2] + ".cw" if parts[-1] == "cw" else parts[-1]
            if key in LC.NEW_FLOORS and v > worst.get(key, (0.0, None))[0]:
                worst[key] = (v, name)
    print("NEW_MEASURE_MAXIMA", worst)
    assert set(worst) == set(LC.NEW_FLOORS)
    for key, (v, name) in worst.items():
        assert 100 * v / LC.STABLE <= LC.NEW_FLOORS[key] <= 100 * v * LC.STABLE, (key, v, name)
    for q in ("x", "dxa", "hist.gap", "aff.mu", "hist.rp_norm"):
        assert LC.floor(q) == LC._bound(q)
    assert LC.floor("hist.sigma") == LC.floor("cor.sigma") == LC.NEW_FLOORS["sigma"] and LC.floor("w.cw") == LC.NEW_FLOORS["w.cw"]


@pytest.mark.parametrize("path", sorted(LC.STOP_SHAPES))
@pytest.mark.parametrize("binding", sorted(LC.STOP_SCALES))
def test_stop_cases_bind_what_they_are_named_after(path, binding):
    case = LC.stop_case(path, binding)
    sides = dict(zip(("rp", "rd", "gap"), LC.stop_sides(case)))
    tau = max(sides.values())
    print("STOP %s/%s %s" % (path, binding, _fmt(sides)))
    assert sides[binding] == tau and all(tau >= 4 * v for k, v in sides.items() if k != binding), sides
    assert IO.converged(case, 2 * tau) and IO.converged(case, tau * (1 + 1e-15)) and not IO.converged(case, tau / 2)
    assert (case.m, case.n) == LC.STOP_SHAPES[path][:2] and case.bounded
