"""The conditions under which tests/test_gpu_small_path_edges.py means something, checked without a GPU (tests/small_path_cases.py
has the builders).

1. Every cell has the structure its name claims: the shape, the tile count and the padding rows of the LDS image; rows of five
   entries or more (tile/); the row-length multiset and the one empty column (rows/); the blockers of the step where stride/ wants
   them, separated from the runner-up by 1e-6 or more in every ratio test (every benign cell); the single column that feeds entry
   (127, 0) of B (list/arrow); the term counts of list/full508 and list/full509 on either side of 2^22, recomputed from the pattern.
2. Every benign cell meets the condition tests/test_iteration_oracle_host.py puts on iteration_oracle's registry: the float64
   restatement of the iteration agrees with the longdouble oracle to 1e-12, the floor of the device's bounds, in the same quantities.
   A cell that misses it is ill-conditioned data: its seed or density changes, never the bound.
3. The late cell is what tests/test_late_cases_host.py asks of late_cases' own: the partition, the residual sizes, the float64 host
   error H in three column orders, the caps on the dropped cells, both oracle solves within H / 100.
   (Of test_late_cases_host's three caps on the dropped cells, the two that speak of one case are asserted: at most 10 % of the
   cells, none of x, s, y in the 2-norm.  The third is about a family keeping a complete case; this cell dropped none on x86-64.)
4. The fire cells fire the test they are built for with the attaining column or row last, and none passes the convergence test.
   The delayed cells fire theirs first at the stop test of iteration K >= 1 of the oracle's trajectory, with a factor sqrt(1.5)
   between every ratio and its tolerance.
"""
import collections

import numpy as np
import pytest

import iteration_oracle as IO
import late_cases as LC
import small_path_cases as SP
from test_iteration_oracle_host import SEPARATION, TOL, _fp64_iteration
from test_gpu_iteration_edges import FLOOR
from test_late_cases_host import DROPPED_SHARE, _fmt


def _shape(name):
    m, n = name.split("/")[1].rstrip("b").split("x")
    return int(m), int(n), name.endswith("b")


def test_the_table_holds_the_cells_the_families_name():
    want = {"tile/" + s for s in ("1x2b", "15x40b", "16x40b", "16x40", "17x40b", "112x300b", "113x300b", "127x300b", "128x300b", "128x300")}
    want |= {"stride/20x%db" % n for n in (511, 512, 513, 1025)} | {"rows/24x64b", "rows/24x64", "list/arrow", "list/full508", "list/full509"}
    assert set(SP.BENIGN) == want
    assert set(SP.DETECT_BENIGN) == {"detect/17x40b", "detect/17x40", "detect/128x300b", "detect/128x300"}
    assert set(SP.FIRE) == {"detect/fire/primal/17x40b/col", "detect/fire/dual/17x40b/row", "detect/fire/dual/17x40b/xu",
                            "detect/fire/primal/16x40/col", "detect/fire/dual/16x40/row", "detect/fire/primal/20x513b/col",
                            "detect/fire/dual/20x513b/row", "detect/fire/dual/20x513b/xu"}
    assert set(SP.CASES) == want | set(SP.DETECT_BENIGN) | set(SP.FIRE) | {SP.LATE_NAME}
    assert not set(SP.CASES) & (set(IO.ITER_CASES) | set(LC.CASES))           # the registries of the other files are untouched
    assert FLOOR == TOL


# ---- structure -------------------------------------------------------------------------------------------------------------
TILES = {"1x2": (1, 15), "15x40": (1, 1), "16x40": (1, 0), "17x40": (2, 15), "112x300": (7, 0), "113x300": (8, 15), "127x300": (8, 1),
         "128x300": (8, 0)}


@pytest.mark.parametrize("name", [nm for nm in SP.BENIGN if nm.startswith("tile/")])
def test_tile_cells(name):
    m, n, bounded = _shape(name)
    case = SP.get(name)
    assert case.A.shape == (m, n) and case.m <= 128 and SP.tiles(m) == TILES["%dx%d" % (m, n)]
    assert case.bounded == bounded and int(case.U.sum()) == (max(1, n // 2) if bounded else 0)
    nz = case.A != 0
    assert nz.any(axis=0).all() and nz.sum(axis=1).min() >= min(SP.MIN_ROW, n), nz.sum(axis=1).min()
    assert m == 1 or nz.mean() < 0.5
    assert np.array_equal(case.b, case.A @ case.xb) and SP.term_count(case.A) <= SP.TERM_LIMIT
    if not bounded:
        twin = SP.get(name + "b")
        assert np.array_equal(case.A, twin.A) and np.array_equal(case.x, twin.x) and not case.w.any() and not case.z.any()


@pytest.mark.parametrize("name", [nm for nm in SP.BENIGN if nm.startswith("stride/")])
def test_stride_cells(name):
    m, n, _ = _shape(name)
    case = SP.get(name)
    assert case.A.shape == (m, n) == (20, n) and SP.tiles(m) == (2, 12) and int(case.U.sum()) == n // 2
    o = IO.iterate(case)
    dual_at = SP.stride_dual_at(n)
    assert dual_at == {511: 0, 512: 0, 513: 511, 1025: 512}[n]            # (513: column 512 is column n - 1, the primal blocker's)
    assert o["argmin_p"][1] == n - 1 and o["argmin_d"][1] == dual_at, (name, o["argmin_p"], o["argmin_d"])
    assert o["ratio_p"] < 1 and o["ratio_d"] < 1                          # they really block
    assert case.U[n - 1]
    assert divmod(n - 1, 512) == {511: (0, 510), 512: (0, 511), 513: (1, 0), 1025: (2, 0)}[n]      # (trip, thread) of the last column
    nz = case.A != 0
    assert nz.any(axis=0).all() and nz.any(axis=1).all()


@pytest.mark.parametrize("name", ["rows/24x64b", "rows/24x64"])
def test_rows_cells(name):
    case = SP.get(name)
    nz = case.A != 0
    assert case.A.shape == (24, 64) and SP.tiles(24) == (2, 8)
    lengths = nz.sum(axis=1)
    assert [int(v) for v in lengths] == [(i % 12) + 1 for i in range(24)]
    assert collections.Counter(int(v) for v in lengths) == {k: 2 for k in range(1, 13)}
    assert np.array_equal(nz[:, :24], np.eye(24, dtype=bool))             # one entry in column i, none elsewhere in the first 24
    d = np.diag(case.A)
    assert np.all((d >= 1.0) & (d < 2.0))
    assert [int(j) for j in np.flatnonzero(~nz.any(axis=0))] == [63]      # the one empty column
    assert case.bounded == name.endswith("b")
    if case.bounded:
        assert case.U[63] and int(case.U.sum()) == 32
    assert np.array_equal(SP.get("rows/24x64b").A, SP.get("rows/24x64").A)


def test_arrow_cell():
    case = SP.get("list/arrow")
    nz = case.A != 0
    assert case.A.shape == (128, 300) and SP.tiles(128) == (8, 0) and case.bounded
    assert nz[:, 0].all()
    for j in range(1, 129):
        assert [int(i) for i in np.flatnonzero(nz[:, j])] == sorted([j - 1, (j + 1) % 128])
    assert np.all(nz[:, 129:].sum(axis=0) == 2)
    both = np.flatnonzero(nz[0] & nz[127])
    assert [int(j) for j in both] == [0]                                  # exactly one column contains both rows 0 and 127
    feeders = (nz[:, None, :] & nz[None, :, :]).sum(axis=2)               # columns that feed entry (i, k) of B
    assert feeders[127, 0] == 1 and feeders.min() == 1 and feeders.max() >= 4        # B is full: 8256 list entries, many of one term
    assert (SP.get("list/full508").A != 0).all()                                      # (the entries fed by hundreds of columns: full508's)
    assert np.array_equal(case.b, case.A @ case.xb) and SP.term_count(case.A) <= SP.TERM_LIMIT


def test_term_counts_on_either_side_of_the_limit():
    c508, c509 = SP.get("list/full508"), SP.get("list/full509")
    assert c508.A.shape == (128, 508) and c509.A.shape == (128, 509) and (c508.A != 0).all() and (c509.A != 0).all()
    assert SP.term_count(c508.A) == 508 * 128 * 129 // 2 == 4194048 <= SP.TERM_LIMIT == 4194304
    assert SP.term_count(c509.A) == 509 * 128 * 129 // 2 == 4202304 > SP.TERM_LIMIT
    assert c508.bounded and c509.bounded


@pytest.mark.parametrize("name", SP.DETECT_BENIGN)
def test_detect_benign_cells_are_tile_cells(name):
    m, n, bounded = _shape(name)
    case = SP.get(name)
    assert case.bounded == bounded and case.A.shape == (m, n)
    assert np.array_equal(case.A, SP.get("tile/%dx%db" % (m, n)).A)


# ---- the oracle's own condition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SP.BENIGN + ["detect/17x40"])
def test_longdouble_oracle_agrees_with_fp64_restatement(name):
    """As tests/test_iteration_oracle_host.py holds iteration_oracle's cases: the same quantities, the same 1e-12."""
    case = SP.get(name)
    o = IO.iterate(case)
    (xn, yn, sn, wn, zn), rec = _fp64_iteration(case, IO.ETA)
    err = {"x": IO.rel(xn, o["xn"]), "s": IO.rel(sn, o["sn"]), "w": IO.rel(wn, o["wn"]), "z": IO.rel(zn, o["zn"]),
           "ATy": IO.rel(case.A.T @ np.ravel(yn), o["atyn"])}
    for k in ("mu", "mu_aff", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "gap", "objective"):
        err[k] = IO.rel(rec[k], o[k])
    err["rp_norm"] = IO.residual_rel(rec["rp_norm"], o["rp_norm"], o["b_norm"])
    err["rd_norm"] = IO.residual_rel(rec["rd_norm"], o["rd_norm"], o["c_norm"])
    print(name, {k: "%.1e" % v for k, v in err.items()})
    assert max(err.values()) <= TOL, (name, err)
    assert not case.bounded or (np.all(o["wn"][~case.U] == 0) and np.all(o["zn"][~case.U] == 0))
    assert o["rp_norm"] > 1e-2 * o["b_norm"] and o["rd_norm"] > 1e-2 * o["c_norm"]       # residual_rel is the plain relative error
    assert o["sigma"] > 1e-6                                                               # a sigma to compare with


@pytest.mark.parametrize("name", SP.BENIGN + ["detect/17x40"])
def test_blockers_are_separated(name):
    o = IO.iterate(SP.get(name))
    for k in ("sep_aff_p", "sep_aff_d", "sep_p", "sep_d"):
        assert o[k] >= SEPARATION, (name, k, o[k])


# ---- the late cell ---------------------------------------------------------------------------------------------------------
def test_late_cell_is_what_it_claims():
    case, mu = SP.get(SP.LATE_NAME), 1e-6
    m, n = case.m, case.n
    assert (m, n) == (128, 300) and SP.tiles(m) == (8, 0) and case.bounded and case.mu_target == mu
    basic, lower, upper = (case.part == p for p in (LC.BASIC, LC.LOWER, LC.UPPER))
    assert int(basic.sum()) == m and int(basic.sum() + lower.sum() + upper.sum()) == n                 # nondeg: |B| = m
    U = case.U
    assert int(U.sum()) == n // 2 and np.all(U[upper]) and 0 < int(upper.sum()) < int(U.sum())
    nz = case.A != 0
    assert nz.any(axis=0).all() and nz.any(axis=1).all() and nz.mean() < 0.15 and SP.term_count(case.A) <= SP.TERM_LIMIT
    ev = SP.late_evaluated()                                                  # (a non-positive pivot of the oracle's Cholesky asserts there)
    o = ev.o
    LD = IO.LD
    rb = case.A.astype(LD) @ case.x.astype(LD) - case.b
    ru = np.where(U, case.x + case.w - np.where(U, case.u, 0.0), 0.0)
    for what, r, data in (("r_b", IO.norm(rb), IO.norm(case.b)), ("r_c", o["rd_norm"], o["c_norm"]), ("r_u", IO.norm(ru), IO.norm(case.u[U]))):
        assert mu / 100 <= float(r / data) <= 100 * mu * np.sqrt(n), (what, float(r / data))
    assert mu / 4 < float(o["mu"]) < 4 * mu
    print("CASE %s cond(B) %.2e mu %.2e" % (SP.LATE_NAME, LC.basis_condition(case), float(o["mu"])))


def test_late_cell_host_error_and_dropped_cells():
    ev = SP.late_evaluated()
    assert len(ev.errs) == 3 and set(ev.H) == set(ev.errs[0]) and all(np.isfinite(v) for v in ev.H.values())
    print("HOST %s\n  H      %s\n  spread %s\n  dropped %s" % (SP.LATE_NAME, _fmt(ev.H), _fmt(ev.spread), sorted(ev.dropped)))
    for k in ev.dropped:
        assert ev.H[k] > LC.floor(k) and ev.spread[k] > LC.STABLE
    assert len(ev.dropped) <= DROPPED_SHARE * len(ev.H)
    assert not ev.dropped & {"x", "s", "y"}, ev.dropped


def test_late_cell_the_two_oracle_solves_agree():
    ev = SP.late_evaluated()
    assert ev.solver is None
    solver = LC.RefinementSolver()
    o2 = IO.iterate(ev.case.copy(), solver=solver)
    assert len(solver.log) == 2 and all(stationary for _, _, stationary in solver.log), solver.log
    e = LC.errors(ev.case, o2, ev.o)
    print("ORACLES %s rounds %s\n  %s" % (SP.LATE_NAME, [r for r, _, _ in solver.log], _fmt(e)))
    bad = {k: (v, ev.H[k]) for k, v in e.items() if not v <= ev.H[k] / 100}
    assert not bad, bad


# ---- the fire cells --------------------------------------------------------------------------------------------------------
def fires(ratios, tol):
    """detect_fire of csrc/iteration_rules.h on (vp / beta, vd / gamma): 5 (the primal test, asked first), 6 or 0."""
    return 5 if ratios[0] <= tol[0] else 6 if ratios[1] <= tol[1] else 0


@pytest.mark.parametrize("name", sorted(SP.DELAYED))
def test_delayed_fire_cells(name):
    """Along the oracle's trajectory nothing fires at the stop tests 0 .. K - 1 and the named test fires at K >= 1, each with a factor
    sqrt(1.5) between ratio and tolerance: the 1e-14 between the device's trajectory and the oracle's cannot move the verdict."""
    d = SP.delayed_fire(name)
    kind, K, tol, ratios, case = d["kind"], d["K"], d["tol"], d["ratios"], d["case"]
    which, margin = (0 if kind == "primal" else 1), np.sqrt(SP.DELAYED_MARGIN)
    assert 1 <= K <= 3 and len(ratios) == len(d["states"]) == K + 1 and all(t > 0 for t in tol) and case.m <= 128
    print("DELAYED %s K %d tol %s ratios %s" % (name, K, tol, ratios))
    for k in range(K):
        assert fires(ratios[k], tol) == 0 and ratios[k][which] >= margin * tol[which] * (1 - 1e-12), (name, k)
    assert fires(ratios[K], tol) == (5, 6)[which] and ratios[K][which] * margin <= tol[which] * (1 + 1e-12)
    assert all(r[1 - which] >= 2 * tol[1 - which] for r in ratios)
    assert not any(IO.converged(at, 1e-8) for at in d["states"])
    q = [IO.infeasibility(at) for at in d["states"]]
    if name.endswith("/xu"):           # the bounded part decides, and an earlier iterate's was larger: a dmxu that is not reset shows
        assert case.bounded and q[K]["vd"] == q[K]["xu_max"] > q[K]["ax_inf"]
        assert max(float(v["xu_max"]) for v in q[:K]) > float(q[K]["xu_max"]) * (1 + 1e-6)
    if kind == "primal":               # u_U . z_U is part of beta, and the earlier iterates' sums are of its size: duz
        U = case.U
        assert case.bounded and q[K]["beta"] > 0
        uz = [float(case.u[U] @ at.z[U]) for at in d["states"]]
        assert min(uz) > 1e-3 * float(q[K]["beta"])
    assert {v[1] for v in SP.DELAYED.values()} == {"primal", "dual"}
    assert not SP.delayed_fire("delayed/dual/128x300")["case"].bounded


@pytest.mark.parametrize("name", SP.FIRE)
def test_fire_cells_fire_their_test(name):
    case = SP.get(name)
    kind = SP.fire_kind(name)
    q = IO.infeasibility(case)
    assert not IO.converged(case, 1e-8)
    assert fires(SP.fire_ratios(case), (0.5, 0.5)) == (5 if kind == "primal" else 6)
    assert case.m <= 128 and case.bounded == name.split("/")[3].endswith("b")
    if kind == "primal":
        assert q["beta"] > 0 and q["vp"] <= 0.5 * q["beta"] and q["vp"] > 0
        assert abs(float(q["beta"] - (4 * q["vp"] + 1))) <= 1e-9 * float(q["beta"])      # beta = 4 vp + 1: a factor 2 inside the tolerance
        assert q["vp"] <= 0.25 * q["beta"]
        assert q["col_p"] == case.n - 1
    else:
        assert q["beta"] <= 0 and q["gamma"] > 0 and q["vd"] <= 0.5 * q["gamma"] and q["vd"] > 0
        if kind == "dual/row":
            assert q["row_d"] == case.m - 1 and q["vd"] == q["ax_inf"] > q["xu_max"]
        else:
            assert q["col_xu"] == case.n - 1 and q["vd"] == q["xu_max"] > q["ax_inf"]
