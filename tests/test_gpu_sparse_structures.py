"""The multifrontal sparse Cholesky (csrc/sparse_chol.h, sparse_symbolic.h, the task partition of host_sparse_setup.h) on
CONSTRUCTED trees at every structural edge, against a longdouble reference with derived bounds.  tests/test_gpu_sparse_factor.py runs
Netlib files only: the regime changes of the kernels then sit wherever Netlib puts them, and the checks there (1e-7 .. 1e-8 against an
oracle that includes the same header) let a dropped update term of relative size 1e-9 pass.

The cases (tests/sparse_cases.py; tests/test_sparse_cases_host.py proves on the CPU that each reaches its edge):
  front | panel mode (r * r <= lds, lds depends on the handle)   clique64 | clique65 (lds 4096), 87 | 88 in clique240_87_88 (lds 7680)
  panel width cut by the LDS budget                               r w = 7680 exactly (32 x 240); w = 31 at r = 241 (clique241)
  MFMA update of panel mode                                       7 and 8 k-steps and the tail step (bigborder_300_20: w = 25, 27, 30,
                                                                  32), one k-step (cstar_70_2_30: w = 2), a last tile with one live row
                                                                  and more tiles than waves (clique65: p = 33)
  extend-add                                                      12 children | 13 with fan-in (star13, cstar_40_3_14 | star14), 8 full
                                                                  groups (star65), 12 groups (star97), two levels with a pass-through
                                                                  single (star106), fan-in in front mode (stars) and in panel mode
                                                                  (cstar_70_2_30, bigborder_300_20, random400), more than 2048 entries
                                                                  in one child (clique240_87_88, bigborder_300_20)
  a child's update vector longer than the workgroup (pc > 256)    bigborder_300_20 (p = 300, 301, 302), in sp_fwd_kernel and in the
                                                                  fused-forward branch of sp_chol_kernel
  tree shape                                                      forests of one-row roots (the padding of every small case), a chain
                                                                  75 panels tall (path300), parent links partly inside a task and partly
                                                                  hand-offs (nd_4_20: 7 tasks among 13 panels; bigborder: 22 among 31)

Bounds (F) on the factor and (S) on the solution: derived in tests/sparse_cases.py, no margin added; the sequential fp64 oracle stays
below 0.04 of (F) and 0.006 of (S) on every case.  Every cell prints its ratios to the bounds (RATIO lines) before it asserts.
One solver is alive at a time (a second live handle switches the walk to level mode) and IPM_SP_MODE is always set explicitly.
Fronts beyond about 5000 rows (where the sweeps' r-vector passes the default dynamic-LDS limit) are out of reach of a test of a few
seconds; the factorization kernel's own raised limit is in use from r = 180 or so (clique240_87_88, clique241, bigborder_300_20).

Largest ratio to (F) / to (S) observed on an MI355X (first run of this file; over both D and both walk modes, which agree bit for bit):
    clique64 0.041 / 0.0061, clique65 0.034 / 0.0070, clique240_87_88 0.015 / 0.0012, clique241 0.026 / 0.0020, star13 0.023 / 0.0053,
    star14 0.022 / 0.0060, star65 0.017 / 0.0046, star97 0.019 / 0.0037, star106 0.014 / 0.0041, cstar_40_3_14 0.033 / 0.0044,
    cstar_70_2_30 0.033 / 0.0032, bigborder_300_20 0.020 / 0.0008, path300 0.014 / 0.0026, nd_4_20 0.023 / 0.0028, random400 0.017 / 0.0030;
    shift: 0.025 / 0.0053, its diagonal 0.025; guard: 0.029 / 0.0048; the iteration of check (e): 1.9e-13 at most (ds), bounds 1e-12 .. 7e-12.
These are for the record: the bounds stay the derived ones.
"""
import numpy as np
import pytest

import interiorpointmethod_amd as ipm

import sparse_cases as SC
import test_gpu_iteration_edges as TE

pytestmark = pytest.mark.gpu

MODES = ("task", "level")
ENV = ("IPM_SP_MODE", "IPM_SP_GRID", "IPM_SP_FUSE_FWD", "IPM_SP_RELAX", "IPM_FACTOR")


def _env(monkeypatch, mode, **more):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IPM_SP_MODE", mode)
    for k, v in more.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _solver(name, **opts):
    A = SC.matrix(name)
    m, n = A.shape
    return ipm.IpmSolver(A, np.zeros(m), np.ones(n), factor="sparse", **opts)


def _check_tree(sv, t, mode):
    fi, sch = sv.factor_info(), sv.schedule()
    assert sv.factor == "sparse" and np.array_equal(sv._perm, t.perm)
    assert (fi["panels"], fi["height"], fi["widest_front"]) == (t.nsn, t.height, t.rmax), fi
    assert fi["tasks"] == t.tasks()[1] and sch["sparse_level_mode"] == (1 if mode == "level" else 0)
    return fi


def _check_clean_walk(sv, mode):
    """The walk itself produced the numbers: no launch fell back to one workgroup, no hand-off timed out."""
    assert sv.factor_info()["serial_launches"] == 0 and sv.schedule()["timeouts_recovered"] == 0


# ---- (a) every case, both scalings, both walks -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", SC.DS)
@pytest.mark.parametrize("name", SC.NAMES)
def test_factor_and_solve_within_the_derived_bounds(name, D, mode, monkeypatch):
    _env(monkeypatch, mode)
    ref = SC.reference(name, D)
    runs = []
    with _solver(name) as sv:
        _check_tree(sv, ref.tree, mode)
        for _ in range(3):
            z = sv.normal_solve(ref.rhs, d=ref.d)
            runs.append((z, sv.get_factor(), sv.last_pivots_fixed))
        _check_clean_walk(sv, mode)
    z, L, fixed = runs[0]
    f, s = SC.check_factor(L, ref), SC.check_solve(z, ref)
    print("RATIO %s D=%g %s F %.4f S %.4f" % (name, D, mode, f, s))
    assert fixed == 0
    assert f <= 1.0 and SC.outside_structure(L, ref) == 0
    assert s <= 1.0
    for z2, L2, fixed2 in runs[1:]:
        assert np.array_equal(z, z2) and np.array_equal(L, L2) and fixed2 == 0


# ---- (b) schedule independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bigborder_300_20", "nd_4_20", "star106", "path300"])
def test_schedule_independence(name, monkeypatch):
    """One workgroup walking the tasks in order, three, the full grid and the level-by-level launches give the same bits."""
    ref = SC.reference(name, 6.0)
    t = ref.tree
    out = []
    for mode, grid in (("task", 1), ("task", 3), ("task", None), ("level", None)):
        _env(monkeypatch, mode, IPM_SP_GRID=grid)
        with _solver(name) as sv:
            fi = _check_tree(sv, t, mode)
            out.append((sv.normal_solve(ref.rhs, d=ref.d), sv.get_factor()))
            _check_clean_walk(sv, mode)
        assert 1 < fi["tasks"] and (fi["tasks"] < fi["panels"] or name == "star106"), fi     # (star106: every panel is its own task)
    for z, L in out[1:]:
        assert np.array_equal(z, out[0][0]) and np.array_equal(L, out[0][1])
    assert SC.check_factor(out[0][1], ref) <= 1.0 and SC.check_solve(out[0][0], ref) <= 1.0


# ---- (c) the Tikhonov shift ------------------------------------------------------------------------------------------------
SHIFT = 2.0 ** -20


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", SC.DS)
@pytest.mark.parametrize("name", ["clique240_87_88", "bigborder_300_20", "star14"])
def test_shift(name, D, mode, monkeypatch):
    """regularize = 2^-20: the factor is that of B_p + shift I with shift = 2^-20 max diag B, on EVERY row (a panel's last column, a
    one-column panel, a root)."""
    _env(monkeypatch, mode)
    ref = SC.reference(name, D, SHIFT)
    with _solver(name, regularize=SHIFT) as sv:
        _check_tree(sv, ref.tree, mode)
        z = sv.normal_solve(ref.rhs, d=ref.d)
        fixed = sv.last_pivots_fixed
        L = sv.get_factor()
        _check_clean_walk(sv, mode)
    f, s, dg = SC.check_factor(L, ref), SC.check_solve(z, ref), SC.shift_ratio(L, ref)
    print("RATIO shift %s D=%g %s F %.4f S %.4f diag %.4f" % (name, D, mode, f, s, dg))
    assert fixed == 0 and f <= 1.0 and s <= 1.0 and dg <= 1.0
    assert SC.outside_structure(L, ref) == 0


# ---- (d) the pivot guard ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SC.GUARD_CASES))
def test_guard(name, mode, monkeypatch):
    """One exactly dependent row: its pivot is zero to rounding (<= 1e-3 of the threshold; every other pivot >= 1e3 of it: asserted on
    the host), so the guarded set is exact.  The guarded column sits, over the cases, first in a panel, last in a 32-wide panel,
    inside a panel-mode and a front-mode panel, in a root, and in a panel with p > 256."""
    _env(monkeypatch, mode)
    g = SC.guard(name)
    ref = g.ref
    with _solver(name, pivot_guard_eps=SC.GUARD_EPS, pivot_guard_big=SC.GUARD_BIG) as sv:
        _check_tree(sv, ref.tree, mode)
        z = sv.normal_solve(ref.rhs, d=ref.d)
        fixed = sv.last_pivots_fixed
        L = sv.get_factor()
        _check_clean_walk(sv, mode)
    dg = np.diag(L)
    assert fixed == len(g.guarded) == 1
    assert np.flatnonzero(dg > 1e30).tolist() == g.guarded.tolist()
    root_big = np.sqrt(SC.GUARD_BIG)
    assert np.all(np.abs(dg[g.guarded] - root_big) <= 2 * np.spacing(root_big))
    zp = np.asarray(z).ravel()[ref.perm]
    assert np.all(np.isfinite(zp)) and np.max(np.abs(zp[g.guarded])) <= 1e-60 * np.linalg.norm(ref.rhs)
    f, s = SC.check_factor(L, ref), SC.check_solve(z, ref)
    print("RATIO guard %s %s F %.4f S %.4f" % (name, mode, f, s))
    assert f <= 1.0 and s <= 1.0 and SC.outside_structure(L, ref) == 0


# ---- (e) one interior-point iteration on the sparse factor -----------------------------------------------------------------
def _bits(*arrays):
    return [None if a is None else np.asarray(a).tobytes() for a in arrays]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bounded", [False, True], ids=["free", "bounded"])
@pytest.mark.parametrize("name", ["bigborder_300_20", "nd_4_20", "star106"])
def test_one_iteration_on_the_sparse_factor(name, bounded, mode, monkeypatch):
    """newton_direction(False), (True) and iterate(1) against the longdouble oracle, element by element, with the helpers and bounds of
    tests/test_gpu_iteration_edges.py; the forward substitution fused into the factorization (IPM_SP_FUSE_FWD=1) and the sweep's own
    kernel (=0) must also agree bit for bit.  bigborder_300_20 puts pc > 256 through both."""
    case = SC.iteration_case(name, bounded)
    t = SC.tree(name)
    bits = {}
    for fuse in ("1", "0"):
        _env(monkeypatch, mode, IPM_SP_FUSE_FWD=fuse)
        with TE._solver(case, as_sparse=True, factor="sparse") as sv:
            _check_tree(sv, t, mode)
            assert sv.sparse and sv.bounded == int(case.U.sum())
            TE.check_iteration("sparse-structure/%s/%s/%s/fuse=%s" % (name, "b" if bounded else "f", mode, fuse), sv, case)
            state = sv.get_state() + (sv.get_bound_state() or (None, None))
            sv.set_state(*case.state())
            dirs = sv.newton_direction(False) + sv.newton_direction(True)
            _check_clean_walk(sv, mode)
        bits[fuse] = _bits(*state) + _bits(*dirs)
    assert bits["1"] == bits["0"]
