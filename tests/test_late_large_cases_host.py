"""The conditions under which tests/test_gpu_late_large.py means something, checked without a GPU (tests/late_large_cases.py has the
cases; every definition -- H, the spread, a dropped cell, the floors, MARGIN, STABLE -- is tests/late_cases.py's).

1. Structure: the block counts, group sizes, leftover block steps and the fused-by-default rule of the table in late_large_cases, from
   the restated group_size, which is held to the library's own at every block count up to 40; the partition sizes of each family.
2. Solvability: refine_oracle.Factor, the host's guarded factor of fl(A Theta A^T), fixes no pivot, and every solve of the oracle's
   RefinementSolver ended stationary.
3. Dropped cells: at most 5 % of all cells over the cases A - D; no case drops a direction or multiplier vector (dxa dya dsa dx dy ds dw
   dz ATdya ATdy y ATy); no benign case drops anything.  A rebuilt case that breaks one of these gets another seed
   (late_large_cases.SEEDS), the rule stays.
4. The bounds mean something: with the deliberately wrong rule theta = x / (s + 1e-14) in the float64 host restatement, at least one
   undropped cell of every late case exceeds its bound.

Observed on x86-64, 8 threads: 315 cells over A - D, none dropped (the CSC case drops alpha_p and its history copy); every refinement
stationary after 3 .. 7 rounds; no pivot fixed.
Condition 4, largest error / bound per case and the next independent cell: A bounded 10.6 (alpha_d; alpha_p, w.cw, x.cw 2.2), A plain
18.2 (alpha_p; sigma 15.1), B 129 (alpha_aff_d; sigma 37), C 6.7 (alpha_d; alpha_aff_d 2.4), D bounded 9.6 (alpha_d; sigma 2.2), D plain
105 (alpha_d; alpha_p 24), the CSC case 15.7 (alpha_d; alpha_aff_d 3.2).  Two replacements were made for this condition
(late_large_cases has the details): the dualdeg cases have a 2 % sparse_pattern A, because with a Gaussian A the ratio was 0.08 .. 0.26;
and a nondeg case at B and primdeg cases at A and D gave 0.05 .. 0.16 at every seed and density tried, so dualdeg cases stand there.

Wall time of the file: printed when its last test has run; 68 s on 8 CPUs, of which about 50 s are the O(m^3) NumPy guarded factors of condition 2.
"""
import ctypes as C
import time

import numpy as np
import pytest

from interiorpointmethod_amd import _lib

import late_cases as LC
import late_large_cases as LL
import qp_oracle as QO
import refine_oracle as RO

DROPPED_SHARE = 0.05
VECTORS = set("dxa dya dsa dx dy ds dw dz ATdya ATdy y ATy".split())
# letter -> (blocks, group size, full groups, leftover block steps, rows of the LP in the last block, fused by default)
TABLE = {"A": (9, 8, 1, 1, 76, False), "B": (12, 4, 3, 0, 128, False), "C": (16, 8, 2, 0, 128, True), "D": (18, 8, 2, 2, 24, True)}


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    """What this file took, the case evaluations included (they are shared: whoever ran first paid)."""
    t0 = time.time()
    yield
    print("\nWALL tests/test_late_large_cases_host.py %.1f s" % (time.time() - t0))


def _fmt(d):
    return " ".join("%s=%.1e" % (k, d[k]) for k in sorted(d))


def test_group_size_is_the_librarys():
    lib = _lib.load()
    count = C.c_int32(0)
    for nb in range(1, 41):
        lay = (C.c_int32 * 4)(0, 0, 0, 0)
        assert lib.ipm_debug_at_pieces(nb, lay, None, 0, C.byref(count)) == _lib.IPM_OK
        assert lay[1] == LL.group_size(nb), nb


@pytest.mark.parametrize("letter", sorted(TABLE))
def test_shape_reaches_what_the_table_says(letter):
    m, n = LL.SHAPES[letter]
    blocks, gsz, groups, leftover, last_rows, fused = TABLE[letter]
    assert LL.blocks_of(m) == blocks == LL.BLOCKS[letter] and blocks > 8
    assert LL.group_size(blocks) == gsz and LL.groups_and_leftover(blocks) == (groups, leftover)
    assert m - 128 * (blocks - 1) == last_rows and LL.fused_by_default(m, n) == fused and m != n
    # IPM_RAGGED_GROUPS=0: groups only where the size divides -- none at 9 and 18 blocks
    assert LL.group_size(blocks, ragged=False) == (gsz if leftover == 0 else 0)
    assert [nm for nm in LL.DENSE if LL.LETTER[nm] == letter and LL.get(nm).A.shape != (m, n)] == []
    # the cases of E: three blocks form no group, eight form one
    assert [LL.group_size(LL.blocks_of(LL.get(nm).m)) for nm in LL.E_CASES] == [0, 0, 8, 8]


@pytest.mark.parametrize("name", LL.NAMES)
def test_case_is_what_it_claims(name):
    kind, shape, family, mu = name.split("/")
    case = LL.get(name)
    m, n = case.m, case.n
    assert LC.IO.shape_name(m, n, case.bounded) == shape and case.mu_target == float(mu) and case.part.shape == (n,)
    U = case.U
    assert int(U.sum()) == (n // 2 if shape.endswith("b") else 0)
    density = float((case.A != 0).mean())
    if LL.is_benign(name):
        assert np.all(case.part == LC.LOWER) and density == 1.0
        theta = case.x / case.s
        assert 0.25 <= theta.min() and theta.max() <= 4.0
    else:
        basic, upper = case.part == LC.BASIC, case.part == LC.UPPER
        assert int(basic.sum()) == m + LC.FAMILIES[family][0]
        assert (0 < int(upper.sum()) < int(U.sum()) and np.all(U[upper])) if case.bounded else not upper.any()
        want = LL.LOCK_DENSITY if kind == "lock" else LL.DUALDEG_DENSITY if family == "dualdeg" else 1.0
        assert abs(density - want) <= 0.05 * want and (case.A != 0).any(axis=0).all() and (case.A != 0).any(axis=1).all()
        o = LL.evaluate(name).o
        assert float(mu) / 4 < float(o["mu"]) < 4 * float(mu)
    print("CASE %s density %.3f |U| %d" % (name, density, U.sum()))


@pytest.mark.parametrize("name", LL.NAMES)
def test_solvable_on_the_host_and_the_oracle_stationary(name):
    ev = LL.evaluate(name)
    case = ev.case
    assert case.m > LC.REFINEMENT_ABOVE and ev.solver is not None
    assert len(ev.solver.log) == 2 and all(stationary for _, _, stationary in ev.solver.log), ev.solver.log
    theta = case.x / case.s
    U = case.U
    theta[U] = 1 / (case.s[U] / case.x[U] + case.z[U] / case.w[U])
    f = RO.Factor(case.A, theta)
    print("SOLVABLE %s refinement %s pivots fixed %d" % (name, ev.solver.log, len(f.fixed)))
    assert not f.fixed, (name, f.fixed)


def test_dropped_cells_stay_inside_the_caps():
    cells = dropped = 0
    for name in LL.NAMES:
        ev = LL.evaluate(name)
        assert len(ev.errs) == 3 and all(np.isfinite(v) for v in ev.H.values()), name
        print("HOST %s\n  H      %s\n  spread %s\n  dropped %s" % (name, _fmt(ev.H), _fmt(ev.spread), sorted(ev.dropped)))
        for k in ev.dropped:
            assert ev.H[k] > LC.floor(k) and ev.spread[k] > LC.STABLE
        assert not ev.dropped & VECTORS, (name, sorted(ev.dropped))
        if LL.is_benign(name):
            assert not ev.dropped, (name, sorted(ev.dropped))
        if name in LL.DENSE:
            cells += len(ev.H)
            dropped += len(ev.dropped)
    print("DROPPED %d of %d cells over A - D: %.1f %%" % (dropped, cells, 100.0 * dropped / cells))
    assert cells == 315 and dropped <= DROPPED_SHARE * cells


@pytest.mark.parametrize("name", LL.LATE)
def test_the_bounds_see_a_wrong_theta(name):
    """x / (s + 1e-14) for x / s in the float64 host restatement: a relative error of 1e-14 / s in theta.  A case that
    stays under every bound is replaced (late_large_cases.py records those that were)."""
    ev = LL.evaluate(name)
    case = ev.case
    e = LC.errors(case, QO.iterate(case, np.zeros(case.n), one_step=False, T=np.float64, theta_shift=1e-14), ev.o)
    bound = LC.bound_of(ev)
    ratio = {k: e[k] / bound(k) for k in e if k not in ev.dropped}
    top = sorted(ratio, key=ratio.get, reverse=True)[:6]
    print("PERTURBED %s error / bound: %s" % (name, " ".join("%s=%.2f" % (k, ratio[k]) for k in top)))
    assert ratio[top[0]] > 1.0, (name, top[0], ratio[top[0]])
