"""The conditions under which tests/test_gpu_iteration_edges.py means something, checked without a GPU.

1. The longdouble oracle of tests/iteration_oracle.py agrees with the two fp64 restatements the suite already trusts
   (oracle.ipm_oracle.iterate(method="normal") without bounds, bounds_oracle.BoundedLP.iterate with bounds) to 1e-12 relative on
   x, s, w, z, A^T y and every scalar, for EVERY case the GPU file uses: fp64 arithmetic alone stays inside every bound of the GPU
   file (1e-12 is the floor of those bounds; the issue's starting bound for the device was 1e-10, 100 x this).  Observed on x86-64: 1e-18 .. 1.3e-13, the worst (sigma) at 520 x 600, where m is close to n.
2. Every GPU case has the property its name promises: the blocker sits where place() put it, in the part (x / w, s / z) the case
   is about, separated from the runner-up by 1e-6 relative or more (rounding cannot swap blockers); the full-step case has a unit
   dual ratio test; the shapes of the dense table reach the chunk counts and block counts they are there for.
3. The infeasibility cases fire the test they are built for, with a factor 2 to spare at tolerance 0.5, and none of them passes
   the convergence test at 1e-8.
"""
import numpy as np
import pytest

import bounds_oracle as BO
import iteration_oracle as IO
from oracle import ipm_oracle as O

TOL = 1e-12
SEPARATION = 1e-6


def _col(v):
    return np.asarray(v, dtype=np.float64).reshape(-1, 1)


def _fp64_iteration(case, eta):
    """(next x, y, s, w, z and the scalars) of the fp64 restatement the suite already has for this kind of case."""
    if case.bounded:
        lp = BO.BoundedLP(case.A, case.b, case.c, case.u)
        xn, yn, sn, wn, zn, rec = lp.iterate(case.x, case.y, case.s, case.w, case.z, eta=eta)
        rp, rd, gap, _, obj = lp.measures(case.x, case.y, case.s, case.w, case.z)
    else:
        x, y, s = _col(case.x), _col(case.y), _col(case.s)
        xn, yn, sn, rec = O.iterate(case.A, _col(case.b), _col(case.c), x, y, s, method="normal", eta=eta)
        rec = dict(rec)
        rec["alpha_aff_p"], rec["alpha_aff_d"] = O.predicted_stepsize(rec["dxa"], rec["dsa"], x, s)
        rc, rb, _ = O.residuals(case.A, _col(case.b), _col(case.c), x, y, s)
        rp, rd, gap, obj = np.linalg.norm(rb), np.linalg.norm(rc), float(case.x @ case.s), float(case.c @ case.x)
        wn, zn = np.zeros(case.n), np.zeros(case.n)
    rec.update(rp_norm=rp, rd_norm=rd, gap=gap, objective=obj)
    return (xn, yn, sn, wn, zn), rec


ETAS = [(name, IO.ETA) for name in sorted(IO.ITER_CASES)] + [("full/" + IO.shape_name(*IO.LARGE, False), 1.0)]


@pytest.mark.parametrize("name,eta", ETAS)
def test_longdouble_oracle_agrees_with_fp64_restatement(name, eta):
    case = IO.get(name)
    o = IO.iterate(case, eta)
    (xn, yn, sn, wn, zn), rec = _fp64_iteration(case, eta)
    err = {"x": IO.rel(xn, o["xn"]), "s": IO.rel(sn, o["sn"]), "w": IO.rel(wn, o["wn"]), "z": IO.rel(zn, o["zn"]),
           "ATy": IO.rel(case.A.T @ np.ravel(yn), o["atyn"])}
    for k in ("mu", "mu_aff", "sigma", "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d", "gap", "objective"):
        err[k] = IO.rel(rec[k], o[k])
    err["rp_norm"] = IO.residual_rel(rec["rp_norm"], o["rp_norm"], o["b_norm"])       # (plain relative errors but for full_step_case)
    err["rd_norm"] = IO.residual_rel(rec["rd_norm"], o["rd_norm"], o["c_norm"])
    print(name, eta, {k: "%.1e" % v for k, v in err.items()})
    assert max(err.values()) <= TOL, (name, err)
    assert not case.bounded or (np.all(o["wn"][~case.U] == 0) and np.all(o["zn"][~case.U] == 0))


@pytest.mark.parametrize("name", sorted(IO.ITER_CASES))
def test_blockers_are_separated(name):
    """Where a ratio test has a blocker at all, the runner-up is at least 1e-6 (relative) behind it: a step length that is off
    because a kernel lost the blocker is off by that much, 1000 x the scalar tolerance of the GPU file."""
    o = IO.iterate(IO.get(name))
    for k in ("sep_aff_p", "sep_aff_d", "sep_p", "sep_d"):
        assert o[k] >= SEPARATION, (name, k, o[k])


PLACED = [nm for nm in sorted(IO.ITER_CASES) if nm.startswith("place/")]


@pytest.mark.parametrize("name", PLACED)
def test_place_puts_the_blocker_where_asked(name):
    which, at = name.rsplit("/", 1)[1].split("@")
    case = IO.get(name)
    o = IO.iterate(case)
    part, col = o["argmin_p" if which == "p" else "argmin_d"]
    assert col == int(at) and col < case.n, (name, part, col)
    assert (o["ratio_p"] if which == "p" else o["ratio_d"]) < 1              # it really blocks
    # nothing but the order of the columns differs from the unplaced case: same multiset of candidates, same step to 1e-15
    base = IO.iterate(IO.get("dense/" + name.split("/")[1]))
    for k in ("alpha_p", "alpha_d", "alpha_aff_p", "alpha_aff_d", "mu", "sigma"):
        assert IO.rel(o[k], base[k]) <= 1e-15, (name, k)


def test_placements_cover_the_edges_of_the_two_level_reduction():
    """Column 0, the last column, the first column of the second block (256) and, past 16384 columns, the last column a thread owns
    alone (16383) and the first of the second grid-stride trip (16384)."""
    names = set(PLACED)
    for which in "pd":
        assert {"place/130x257b/%s@%d" % (which, at) for at in (0, 256)} <= names
        assert {"place/129x16385b/%s@%d" % (which, at) for at in (0, 256, 16383, 16384)} <= names


@pytest.mark.parametrize("name,key", [("blocker/130x257b/w", "argmin_p"), ("blocker/129x16385b/w", "argmin_p"),
                                      ("blocker/130x257b/z", "argmin_d"), ("blocker/130x257b/zaff", "argmin_aff_d"),
                                      ("blocker/129x16385b/zaff", "argmin_aff_d")])
def test_bound_part_blockers(name, key):
    """The blocker is a w (z) component, in the last column.  z blocks the STEP at 130 x 257 only; at 129 x 16385 it blocks the affine
    ratio test (raise_bound), which is the same kernel code with corr = 0 and shows in alpha_aff_d."""
    case = IO.get(name)
    o = IO.iterate(case)
    assert o[key] == (1, case.n - 1), (name, o[key])
    assert case.U[case.n - 1]
    assert o[{"argmin_p": "ratio_p", "argmin_d": "ratio_d", "argmin_aff_d": "alpha_aff_d"}[key]] < 1


def test_full_step_case_has_a_unit_dual_step():
    """No component of s decreases enough to block: both dual ratio tests return exactly 1 (the initial value of min_partials), the
    primal ones stay below 1.  The step is min(1, eta * ratio): exactly eta at the default eta = 0.91, exactly 1.0 only at eta = 1."""
    case = IO.get("full/" + IO.shape_name(*IO.LARGE, False))
    assert (case.m, case.n) == IO.LARGE and not case.bounded
    o1, o = IO.iterate(case, 1.0), IO.iterate(case)
    assert o1["alpha_d"] == 1.0 and o1["alpha_aff_d"] == 1.0 and o1["ratio_d"] == 1.0
    assert o1["alpha_p"] < 1 and o1["alpha_aff_p"] < 1
    assert float(o["alpha_d"]) == 0.91 and o["alpha_p"] < 0.91
    assert o["cand_d"].min() > 1 and o["cand_aff_d"].min() > 1           # every candidate is beyond the unit step, none equals it


def test_one_by_one_case_has_no_blocker():
    """Every ratio test returns its initial 1: the one candidate each has lies beyond the unit step.  (With one column the affine
    direction has dx/x + ds/s = -1; a seed whose affine step is blocked has mu_aff = 0 to rounding, and no sigma to compare with.)"""
    o = IO.iterate(IO.get("dense/1x1"))
    for k in ("cand_aff_p", "cand_aff_d", "cand_p", "cand_d"):
        assert o[k].min() > 1, k
    assert o["alpha_aff_p"] == 1 and o["alpha_aff_d"] == 1 and float(o["alpha_p"]) == 0.91 and float(o["alpha_d"]) == 0.91
    assert o["sigma"] > 1e-3


def _layout(m, n, sparse=False):
    """make_layout of csrc/host_handle.h, the part the vector kernels see (m < 2048: no extra padding of mp)."""
    mp, np_ = -(-m // 128) * 128, -(-n // 64) * 64
    return dict(mp=mp, np=np_, rc_chunks=1 if sparse else min(32, mp // 64), vblk=min(64, max(1, -(-max(m, n) // 256))))


def test_dense_table_reaches_what_it_is_there_for():
    L = {(m, n): _layout(m, n) for m, n, _ in IO.DENSE_TABLE}
    assert L[(3, 64)]["np"] == 64 and L[(3, 64)]["rc_chunks"] == 2
    assert L[(5, 65)]["np"] == 128
    assert L[(130, 257)]["rc_chunks"] == 4 and L[(130, 257)]["vblk"] == 2
    assert L[(300, 513)]["rc_chunks"] == 6 and L[(300, 513)]["vblk"] == 3 and L[(300, 513)]["np"] == 576
    assert L[(400, 520)]["rc_chunks"] == 8 and L[(400, 520)]["vblk"] == 3
    assert L[(520, 600)]["rc_chunks"] == 10
    assert L[(129, 16384)]["vblk"] == 64 and 64 * 256 == 16384
    assert L[(129, 16385)]["vblk"] == 64 and 16385 > 64 * 256
    bounded = {(m, n): bd for m, n, bd in IO.DENSE_TABLE}
    assert [bounded[k] for k in ((1, 1), (3, 64), (5, 65), (130, 257), (300, 513), (400, 520), (520, 600), (129, 16384), (129, 16385))] == \
        [False, False, True, True, False, True, False, False, True]
    for m, n, bd in IO.DENSE_TABLE:
        case = IO.get("dense/" + IO.shape_name(m, n, bd))
        assert case.A.shape == (m, n) and int(case.U.sum()) == (max(1, n // 2) if bd else 0)
        if bd:
            assert np.all(IO.iterate(case)["rp_norm"] > 0) and np.any(case.x[case.U] + case.w[case.U] != case.u[case.U])    # r_u != 0


@pytest.mark.parametrize("name", ["sparse/5x65b", "sparse/130x257b", "sparse/129x16385b", "lock/130x257", "lock/129x16385"])
def test_sparsified_cases(name):
    case = IO.get(name)
    nz = case.A != 0
    assert nz.any(axis=0).all() and nz.any(axis=1).all()
    assert nz.mean() < 0.1 or case.m <= 5          # (5 x 65: one entry per column is already 20 %)
    assert np.array_equal(case.b, case.A @ case.xb)
    assert case.bounded == name.startswith("sparse/")


@pytest.mark.parametrize("name", sorted(IO.FIRE_CASES))
def test_infeasibility_cases_fire_their_test(name):
    case = IO.get("fire/" + name)
    q = IO.infeasibility(case)
    assert not IO.converged(case, 1e-8)
    if name.startswith("primal/"):
        assert q["beta"] > 0 and q["vp"] <= 0.5 * q["beta"] and q["vp"] > 0
        assert abs(float(q["vp"] / q["beta"]) - 0.25) < 0.01                   # beta = 4 vp + 1: a factor 2 inside the tolerance
    else:
        assert q["beta"] <= 0 and q["gamma"] > 0 and q["vd"] <= 0.5 * q["gamma"] and q["vd"] > 0
    where = name.rsplit("/", 1)[1]
    if where.startswith("col@"):
        assert q["col_p"] == int(where[4:]) == case.n - 1
    elif where.startswith("row@"):
        assert q["row_d"] == int(where[4:]) == case.m - 1 and q["vd"] == q["ax_inf"] > q["xu_max"]
    elif where.startswith("xu@"):
        assert q["col_xu"] == int(where[3:]) == case.n - 1 and q["vd"] == q["xu_max"] > q["ax_inf"]


def test_infeasibility_cases_cover_both_kernels_and_both_shapes():
    names = set(IO.FIRE_CASES)
    for shape in ("130x257", "129x16385"):
        for b in ("", "b"):
            assert any(nm.startswith("primal/%s%s/" % (shape, b)) for nm in names)
            assert any(nm.startswith("dual/%s%s/row@" % (shape, b)) for nm in names)
        assert any(nm.startswith("dual/%sb/xu@" % shape) for nm in names)
    assert {"primal/sparse130x257", "dual/sparse130x257"} <= names
