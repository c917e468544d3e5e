"""GPU tests (-m gpu) of the iterative refinement of the normal-equations solves (csrc/iteration_rules.h refine_decide,
csrc/refine_ops.h, host_iteration.h enqueue_refine).  The rule, its input families and the extended-precision
reference are tests/refine_oracle.py; tests/test_refine_oracle_host.py shows on the CPU that every case used here meets, of the
oracle alone, what is asserted of the device below, and drops the cases that do not.

1. Forward error ||dy - ref|| / ||ref|| against the np.longdouble reference, through normal_solve(rhs, d) and through
   newton_direction (set_state with x = d 2^-140, s = 2^-140, y = 0, b = t, c = s: then x / s = d bitwise, r_c = 0, v = -x, and
   A x is below half an ulp of every t_i, so the predictor's right-hand side is t bitwise), on a dense handle, a sparse-A handle
   and a bounded handle: the error at k = 0 exceeds 100 x the error at k = 2, and the error at k = 2 is within 16 x the oracle's
   for the same input.  (Bounded newton_direction: theta = 1 / (s/x + z/w) is computed by the device;
   refine_oracle.get_theta restates it and the cases are evaluated, and kept or dropped, like all others.)  No fixed tolerance.
2. regularize = 1e-6 on the cond ~ 4e1 family: k = 2 agrees with the regularize = 0, k = 0 solve within the same bound, k = 0 does not.
3. Shapes m = 1, 127, 128, 129 (grouped sweeps), 257; 16 blocks with streamed A^T dy against IPM_STREAM_AT=0 bit for bit;
   IPM_FUSED_FACTOR=force; the smallest tree of tests/sparse_cases.py on the sparse factor through normal_solve, and SC205 on the
   sparse factor through iterate(), where the predictor's forward sweep rides on the factorization and the rounds must not
   (bitwise the run with IPM_SP_FUSE_FWD=0).  Each is bitwise repeatable, gives the same bytes on memory that held 0xFF, and the
   padding rows of t, r, delta and dy (ipm_debug_get_refine_vector) read back as exact zeros.
4. Guarded pivots: a tests/guard_cases.py case with a consistent right-hand side (error at k = 2 at most the error at k = 0, no
   revert), and the duplicated row with an inconsistent one (half rule or revert, residual not above k = 0's).
5. Off means off.  6. check_every 1 against 7.  7. With centrality correctors.  8. SC205 end to end.  9. Refusals.

Measured on MI355X (forward error of the device at k = 0 / k = 2, then the oracle's at k = 2; dense
handle, normal_solve, 130 x 260; the same figures to two digits through newton_direction and on the sparse-A and bounded handles):
    p0-shift1e-6   9.2e-06 / 1.5e-15   1.5e-15        p4-shift1e-8   1.8e-04 / 7.2e-12   7.2e-12
    p4-shift0      8.6e-12 / 9.2e-16   6.9e-16        p8-shift0      3.6e-07 / 9.6e-16   8.6e-16
    p8-shift1e-12  6.9e-04 / 4.0e-10   4.0e-10
  over all 75 cells the device's error at k = 2 is at most 1.52 x the oracle's (p4-shift0/130x173: 1.26e-15 against 8.3e-16), and
  the smallest gain k = 0 over k = 2 is 478 (p4-shift1e-8/130x173: 3.9e-02 -> 8.1e-05).  Shifted factor (test 2): against the
  regularize = 0 solve, k = 0 differs by 9.2e-06 and 6.5e-06, k = 2 by 1.4e-15 and 1.7e-15 (bounds 2.4e-14, 1.4e-14).
  Inconsistent duplicated row: residual 1.0000000000000007 at k = 0, 0.99999999999999989 at k = 3, one correction, one half-rule end.
"""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batch, batches
from interiorpointmethod_amd.handle import RefineInfo
from interiorpointmethod_amd.matio import load_npz_problem
from interiorpointmethod_amd.workloads import synthetic_lp

import guard_cases as GC
import refine_oracle as R
import sparse_cases as SC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
KEPT = R.kept_cases()
ROWS = [k for k in KEPT if (k[1], k[2]) in ((130, 260), (257, 515))]          # the five table rows at two sizes
_id = lambda k: "%s-%dx%d" % k          # noqa: E731
TINY = 2.0 ** -140


def _ub(c, kind):
    if kind != "bounded":
        return None
    u = np.full(c.n, np.inf)
    u[::3] = 1.0
    return u


def _make(c, kind, refine=0, shift=None, **kw):
    A = sparse.csc_matrix(c.A) if kind == "sparse" else c.A
    return ipm.IpmSolver(A, c.t, np.ones(c.n), ub=_ub(c, kind), regularize=c.shift if shift is None else shift, refine=refine, **kw)


def _check_kind(sv, kind):
    sch = sv.schedule()
    assert sch["fused_small"] == 0 and sv.sparse == (kind == "sparse") and bool(sv.bounded) == (kind == "bounded"), (kind, sch)


def _assert_forward(tag, c, e0, e2, oracle2):
    msg = "%s: forward error k=0 %.3e, k=2 %.3e; oracle k=2 %.3e (k=0 %.3e)" % (tag, e0, e2, oracle2, c.err[0])
    print("ERR " + msg)
    assert e0 > R.GAIN * e2, msg
    assert e2 <= R.ORACLE_MARGIN * oracle2, msg


# ---- 1. forward error --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", [("dense", k) for k in KEPT] + [(kd, k) for kd in ("sparse", "bounded") for k in ROWS],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_forward_error_normal_solve(kind, key):
    c = R.get(*key)
    with _make(c, kind) as sv:
        _check_kind(sv, kind)
        e = {}
        for k in (0, 2):
            sv.set_refine(k)
            e[k] = R.forward_error(sv.normal_solve(c.t, d=c.d), c.ref)
            info = sv.refine_info()
            assert info.k == k and info.solves == (1 if k else 0) and info.reverts == 0, info
        assert info.applied >= 1 and info.first_rel > 0.0 and info.max_first_rel == info.first_rel, info
    _assert_forward("normal_solve/%s/%s" % (kind, c.name), c, e[0], e[2], c.err[2])


def _direction_state(c):
    """x = d 2^-140, s = 2^-140, y = 0 (module docstring)."""
    return c.d * TINY, np.zeros(c.m), np.full(c.n, TINY)


THETA_ROWS = [k for k in ROWS if R.oracle_meets(R.get_theta(*k))]          # (the bounded handle's cases, held to the same predicate)


@pytest.mark.parametrize("kind,key", [(kd, k) for kd in ("dense", "sparse") for k in ROWS] + [("bounded", k) for k in THETA_ROWS],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_forward_error_newton_direction(kind, key):
    c = R.get_theta(*key) if kind == "bounded" else R.get(*key)
    x, y, s = _direction_state(R.get(*key))
    A = sparse.csc_matrix(c.A) if kind == "sparse" else c.A
    ub, w, z = None, None, None
    if kind == "bounded":
        # on U: w = z = 2^-140 = s and u = x + w (r_u = 0), so theta = 1 / (s/x + z/w) = 1 / (1/d + 1) in the device's own expression
        # (refine_oracle.get_theta restates it); c = s - z on U keeps r_c = 0, and v = theta (r_c - s + z) = 0 there, so the
        # right-hand side is t + A_notU x = t bitwise.
        U = R.bounded_columns(c.n)
        w, z = np.where(U, TINY, 0.0), np.where(U, TINY, 0.0)
        ub = np.where(U, x + TINY, np.inf)
    cvec = s - (z if z is not None else 0.0)
    e = {}
    with ipm.IpmSolver(A, c.t, cvec, ub=ub, regularize=c.shift) as sv:
        _check_kind(sv, kind)
        for k in (0, 2, 2):          # (twice with k = 2: the tallies are those of the call, not a running count)
            sv.set_refine(k)
            sv.set_state(x, y, s, w=w, z=z)
            _, dy, _ = sv.newton_direction(corrector=False)
            e[k] = R.forward_error(dy.ravel(), c.ref)
            assert sv.refine_info().solves == (1 if k else 0)
    _assert_forward("newton_direction/%s/%s" % (kind, c.name), c, e[0], e[2], c.err[2])


# ---- 2. the shifted factor ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in ROWS if k[0] == "p0-shift1e-6"], ids=_id)
def test_refinement_removes_the_shift(key):
    c = R.get(*key)
    with _make(c, "dense", shift=0.0) as sv:
        plain = sv.normal_solve(c.t, d=c.d)
    with _make(c, "dense", shift=1e-6) as sv:
        got = {}
        for k in (0, 2):
            sv.set_refine(k)
            got[k] = R.forward_error(sv.normal_solve(c.t, d=c.d), np.asarray(plain, dtype=R.LD))
    bound = R.ORACLE_MARGIN * c.err[2]
    msg = "%s: against regularize=0, k=0: k=0 %.3e, k=2 %.3e, bound 16 x oracle %.3e" % (c.name, got[0], got[2], bound)
    print("SHIFT " + msg)
    assert got[2] <= bound, msg
    assert not got[0] <= bound, msg


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------
def _shape_case(m, n, seed):
    rng = np.random.default_rng([7, m, n, seed])
    A = rng.standard_normal((m, n))
    d = np.exp(rng.uniform(-np.log(1e4), np.log(1e4), n))
    return A, d, rng.standard_normal(m)


def _assert_padding_zero(sv, dy="dy"):
    """Rows m .. mp-1 of t, r, delta and dy of the last refined solve, read back whole: exactly zero."""
    for which in ("t", "r", "delta", dy):
        v = sv.debug_refine_vector(which)
        assert v.shape[0] >= sv.m and v.shape[0] % 128 == 0, (which, v.shape)
        pad = v[sv.m:]
        assert np.all(pad == 0.0), (which, sv.m, v.shape[0], pad[np.nonzero(pad != 0.0)][:4])
    return v.shape[0]


def _twice_and_on_nan_memory(monkeypatch, make, run):
    """run(sv) -> bytes-comparable result: twice on one handle, on a fresh one, and on a fresh one whose memory held 0xFF."""
    out = []
    with make() as sv:
        out += [run(sv), run(sv)]
    monkeypatch.setenv("IPM_TEST_ALLOC_FILL", "255")
    with make() as sv:
        out.append(run(sv))
    monkeypatch.delenv("IPM_TEST_ALLOC_FILL")
    assert out[0] == out[1] == out[2]
    return out[0]


@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_shapes_dense(m, monkeypatch):
    n = 2 * m + 3
    A, d, t = _shape_case(m, n, 0)

    def run(sv):
        z = sv.normal_solve(t, d=d)
        assert np.all(np.isfinite(z))
        assert _assert_padding_zero(sv) == 128 * ((m + 127) // 128)
        return z.tobytes(), tuple(sv.refine_info())

    make = lambda k=2: ipm.IpmSolver(A, t, np.ones(n), regularize=1e-8, refine=k)          # noqa: E731
    with make(0) as sv:
        sch = sv.schedule()
        assert not sv.sparse and sch["fused_small"] == 0 and sch["blocks"] == (m + 127) // 128
        if m == 129:
            assert sch["grouped_trsv"] == 1          # two blocks: one group of two, the grouped sweeps
        z0 = sv.normal_solve(t, d=d)
    zb, info = _twice_and_on_nan_memory(monkeypatch, make, run)
    info = RefineInfo(*info)
    z2 = np.frombuffer(zb)
    r0, r2 = R.residual_norm(A, d, t, z0), R.residual_norm(A, d, t, z2)
    print("SHAPE m=%d residual k=0 %.3e k=2 %.3e info %s" % (m, r0, r2, info))
    assert info.solves == 1 and info.applied >= 1 and info.reverts == 0
    assert r2 < r0


def test_streamed_at_is_bit_identical_to_unstreamed(monkeypatch):
    A, b, c = synthetic_lp(2040, 2304, seed=7)          # (16 blocks with eight padding rows)

    def run(sv):
        sv.init_state(0.0)
        st = sv.iterate(3)
        _assert_padding_zero(sv, "dy")
        _assert_padding_zero(sv, "dya")
        return [v.tobytes() for v in sv.get_state()], sv.history(), tuple(sv.refine_info()), st["iterations"]

    with ipm.IpmSolver(A, b, c, refine=2) as sv:
        first, again = run(sv), run(sv)
        sch = sv.schedule()
    assert sch["blocks"] == 16 and sch["stream_at"] == 1 and sch["timeouts_recovered"] == 0, sch
    assert first == again and first[3] == 3 and first[2][1] == 6 and first[2][2] >= 1, first[2]
    monkeypatch.setenv("IPM_STREAM_AT", "0")
    with ipm.IpmSolver(A, b, c, refine=2) as sv:
        single = run(sv)
        assert sv.schedule()["stream_at"] == 0
    assert single == first


def test_fused_factor_launch(monkeypatch):
    monkeypatch.setenv("IPM_FUSED_FACTOR", "force")
    A, b, c = synthetic_lp(300, 640, seed=3)

    def run(sv):
        sv.init_state(0.0)
        sv.iterate(3)
        assert sv.schedule()["fused_factor"] == 1
        _assert_padding_zero(sv, "dy")
        _assert_padding_zero(sv, "dya")
        return [v.tobytes() for v in sv.get_state()], sv.history(), tuple(sv.refine_info())

    got = _twice_and_on_nan_memory(monkeypatch, lambda: ipm.IpmSolver(A, b, c, refine=2), run)
    assert got[2][1] == 6 and got[2][4] == 0, got[2]
    assert all(np.all(np.isfinite(np.frombuffer(v))) for v in got[0])


def test_sparse_factor_smallest_tree(monkeypatch):
    name = "clique64"          # one clique: the smallest panel tree of tests/sparse_cases.py
    A = SC.matrix(name)
    m, n = A.shape
    d, t = SC.dvec(name, 2), SC.rhs(name)

    def run(sv):
        z = sv.normal_solve(t, d=d)
        _assert_padding_zero(sv)
        return z.tobytes(), tuple(sv.refine_info())

    make = lambda k=2: ipm.IpmSolver(A, t, np.ones(n), factor="sparse", regularize=1e-8, refine=k)          # noqa: E731
    with make(0) as sv:
        assert sv.sparse and sv.factor == "sparse" and sv.factor_info()["panels"] >= 1
        z0 = sv.normal_solve(t, d=d)
    zb, info = _twice_and_on_nan_memory(monkeypatch, make, run)
    Ad = A.toarray()
    r0, r2 = R.residual_norm(Ad, d, t, z0), R.residual_norm(Ad, d, t, np.frombuffer(zb))
    print("SPARSE-FACTOR residual k=0 %.3e k=2 %.3e info %s" % (r0, r2, info))
    assert info[1] == 1 and info[2] >= 1 and info[4] == 0 and r2 < r0


def test_sparse_factor_iteration_uses_the_plain_substitution(monkeypatch):
    """On the sparse factor the predictor's forward sweep rides on the factorization (IPM_SP_FUSE_FWD=1, the default); the rounds
    behind that solve substitute with the plain forward + backward sweep.  iterate(3) with k = 2 is bitwise repeatable and bitwise
    the run with IPM_SP_FUSE_FWD=0, where the predictor's own solve is the plain sweep too."""
    A, b, c = _netlib("SC205")
    out = {}

    def run(sv):
        assert sv.factor == "sparse" and sv.factor_info()["panels"] >= 1
        sv.init_state(1.0)
        assert sv.iterate(3)["iterations"] == 3
        _assert_padding_zero(sv, "dy")
        _assert_padding_zero(sv, "dya")
        return _bits(sv), sv.history(), tuple(sv.refine_info())

    for fuse in ("1", "0"):
        monkeypatch.setenv("IPM_SP_FUSE_FWD", fuse)
        out[fuse] = _twice_and_on_nan_memory(monkeypatch, lambda: ipm.IpmSolver(A, b, c, factor="sparse", refine=2), run)
    assert out["1"] == out["0"] and out["1"][2][1] == 6 and out["1"][2][2] >= 6, out["1"][2]


# ---- 4. guarded pivots -------------------------------------------------------------------------------------------------------
def test_guarded_pivots_consistent_rhs():
    g = GC.GuardCase(130, seed=2)
    B = g.B()
    rng = np.random.default_rng(11)
    z0 = np.zeros(g.m)
    z0[g.keep] = rng.integers(-3, 4, g.keep.size).astype(np.float64)
    rhs = B @ z0          # consistent: in the range of the kept rows' columns
    want = g.reduced_solution(B, rhs)
    err = {}
    with ipm.IpmSolver(g.A, rhs, np.ones(g.n)) as sv:
        for k in (0, 2):
            sv.set_refine(k)
            z = sv.normal_solve(rhs, d=g.d)
            assert sv.last_pivots_fixed == len(g.guarded)
            err[k] = float(np.linalg.norm(z - want) / np.linalg.norm(want))
            info = sv.refine_info()
    print("GUARD consistent: error k=0 %.3e k=2 %.3e info %s" % (err[0], err[2], info))
    assert err[2] <= err[0] and info.reverts == 0 and info.solves == 1, (err, info)


def test_guarded_pivot_inconsistent_rhs_ends_the_rounds():
    D = R.DuplicatedRow()
    t = D.inconsistent()
    res = {}
    with ipm.IpmSolver(D.A, t, np.ones(D.n), pivot_guard_eps=D.eps) as sv:
        for k in (0, 3):
            sv.set_refine(k)
            z = sv.normal_solve(t, d=D.d)
            assert sv.last_pivots_fixed == 1
            res[k] = R.residual_norm(D.A, D.d, t, z)
            info = sv.refine_info()
    print("GUARD inconsistent: residual k=0 %.17g k=3 %.17g info %s" % (res[0], res[3], info))
    assert info.half_rule + info.reverts >= 1 and info.applied == 1 and info.solves == 1, info
    assert res[3] <= res[0], (res, info)


# ---- 5. off means off --------------------------------------------------------------------------------------------------------
def _bits(sv):
    return [v.tobytes() for v in sv.get_state()]


@pytest.mark.parametrize("as_sparse", [False, True])
def test_off_means_off(as_sparse):
    A, b, c = synthetic_lp(130, 260, seed=5)
    if as_sparse:
        A = sparse.csc_matrix(A)
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        assert sv.iterate(5)["iterations"] == 5
        want = (_bits(sv), sv.history())
        assert tuple(sv.refine_info()) == (0,) * 8
    with ipm.IpmSolver(A, b, c) as sv:
        sv.set_refine(2)
        sv.set_refine(0)
        sv.init_state(0.0)
        sv.iterate(5)
        assert (_bits(sv), sv.history()) == want and tuple(sv.refine_info()) == (0,) * 8
    with ipm.IpmSolver(A, b, c, refine=2) as sv:          # a handle that RAN rounds, set back
        sv.init_state(0.0)
        sv.iterate(2)
        assert sv.refine_info().solves == 4
        sv.set_refine(0)
        sv.init_state(0.0)
        sv.iterate(5)
        assert (_bits(sv), sv.history()) == want and tuple(sv.refine_info()) == (0,) * 8


# ---- 6. no dependence on how far the host runs ahead -------------------------------------------------------------------------
def _netlib(name):
    A, b, c, _, _ = load_npz_problem(os.path.join(GOLDEN, "netlib", name + ".npz"))
    return sparse.csc_matrix(A, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel()


@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_check_every_does_not_change_a_bit(which, monkeypatch):
    monkeypatch.delenv("IPM_CHECK_EVERY", raising=False)
    A, b, c = synthetic_lp(200, 520, seed=9) if which == "dense" else _netlib("SC205")
    out = []
    for ce in (1, 7):
        with ipm.IpmSolver(A, b, c, check_every=ce, refine=2) as sv:
            sv.init_state(0.0 if which == "dense" else 1.0)
            st = sv.solve(tol=1e-8, max_iter=200)
            out.append((_bits(sv), sv.history(), tuple(sv.refine_info()), st["status"], st["iterations"]))
    print("RUN-AHEAD %s status %d iterations %d info %s" % (which, out[0][3], out[0][4], out[0][2]))
    assert out[0] == out[1] and out[0][3] == 1 and out[0][2][1] == 2 * out[0][4]


# ---- 7. with centrality correctors -------------------------------------------------------------------------------------------
def test_every_solve_that_did_work_is_refined():
    A, b, c = synthetic_lp(200, 520, seed=9)
    with ipm.IpmSolver(A, b, c, correctors=2, refine=1) as sv:
        sv.init_state(0.0)
        st = sv.iterate(6)
        ci, ri = sv.corrector_info(), sv.refine_info()
    print("MCC+REFINE correctors %s refine %s" % (ci, ri))
    assert st["iterations"] == 6 and ci["rounds"] >= 6
    assert ri[1] == 2 * 6 + ci["rounds"], (ri, ci)


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["reference", "mehrotra"])
def test_sc205_end_to_end(start):
    A, b, c = _netlib("SC205")
    assert A.shape[0] > 128
    tol, runs = 1e-8, {}
    for k in (0, 2):
        x, y, s, info = ipm.solve_with_info(A, b, c, tol=tol, max_iter=500, start=start, refine=k)
        assert info["status"] == 1 and info["refine"].k == k, info
        assert (info["refine"].solves == 2 * info["iterations"]) if k else tuple(info["refine"]) == (0,) * 8
        runs[k] = (info["objective"], info["iterations"], info["refine"])
    diff, bound = abs(runs[0][0] - runs[2][0]), tol * (1.0 + abs(runs[0][0]))
    msg = "SC205 start=%s iterations k=0 %d, k=2 %d; objective %.15e, |difference| %.3e, tol (1 + |objective|) %.3e; refine %s" % (
        start, runs[0][1], runs[2][1], runs[0][0], diff, bound, runs[2][2])
    print("E2E " + msg)
    assert diff <= bound, msg


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    rng = np.random.default_rng(3)
    As = sparse.csc_matrix(np.hstack([np.eye(5), rng.standard_normal((5, 60))]))
    bs, cs = np.asarray(As @ np.ones(65)).ravel(), np.ones(65)
    with ipm.IpmSolver(As, bs, cs) as sv:
        assert sv.schedule()["fused_small"] == 1
        with pytest.raises(_lib.IpmError, match="small"):
            sv.set_refine(1)
        assert sv.refine == 0 and sv.refine_info().k == 0
        sv.init_state(1.0)
        assert sv.iterate(1)["iterations"] == 1
    with pytest.raises(_lib.IpmError, match="small"):
        ipm.IpmSolver(As, bs, cs, refine=1)
    A, b, c = _netlib("SC205")
    with ipm.IpmSolver(A, b, c, lockstep=True, factor="dense") as sv:
        with pytest.raises(_lib.IpmError, match="LOCKSTEP"):
            sv.set_refine(1)
        sv.init_state(1.0)
        with pytest.raises(ValueError, match="refine"):
            ipm.solve_lockstep([sv], tol=1e-8, max_iter=2, refine=1)
        assert ipm.solve_lockstep([sv], tol=1e-8, max_iter=2)[0]["iterations"] == 2
    # a handle moved to the small path after k > 0 (ipm_set_A_csc decides the path: 600 dense columns of 128 rows are past the
    # product-list cap of the one-workgroup kernel, the sparse matrix of the same shape is not): the solve entries refuse until k = 0
    m, n = 128, 600
    Ab = rng.standard_normal((m, n))
    Ab[:, :m] += 4.0 * np.eye(m)
    cols = np.arange(m, n)
    Asm = sparse.csc_matrix((np.ones(m + 2 * cols.size), (np.concatenate([np.arange(m), cols % m, (7 * cols + 1) % m]),
                                                          np.concatenate([np.arange(m), cols, cols]))), shape=(m, n))
    Asm.sort_indices()
    with ipm.IpmSolver(sparse.csc_matrix(Ab), Ab @ np.ones(n), np.ones(n), reorder=None, refine=1) as sv:
        assert sv.schedule()["fused_small"] == 0 and sv._perm is None
        indptr, indices, data = Asm.indptr.astype(np.int32), Asm.indices.astype(np.int32), Asm.data.astype(np.float64)
        sv._check(sv._lib.ipm_set_A_csc(sv._h, indptr.ctypes.data_as(C.POINTER(C.c_int32)), indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                        data.ctypes.data_as(C.POINTER(C.c_double)), int(data.shape[0])))
        assert sv.schedule()["fused_small"] == 1 and sv.refine_info().k == 1
        sv.init_state(1.0)
        for call in (lambda: sv.iterate(1), lambda: sv.solve(max_iter=2), lambda: sv.newton_direction(), lambda: sv.normal_solve(np.ones(m))):
            with pytest.raises(_lib.IpmError, match="small"):
                call()
        sv.set_refine(0)
        assert sv.iterate(1)["iterations"] == 1
    for k in (-1, _lib.MAX_REFINE + 1):
        with pytest.raises(ValueError, match="refine"):
            ipm.IpmSolver(A, b, c, refine=k)
        assert _lib.load().ipm_set_refinement(None, k) != 0
    with pytest.raises(ValueError, match="refine"):
        ipm.solve_small_batch([(As, bs, cs)], refine=1)
    with pytest.raises(ValueError, match="refine"):
        batches.solve_small_batch_solvers([], refine=1)
    with pytest.raises(ValueError, match="refine"):
        batch.solve_shard_lockstep([(A, b, c)], [0], refine=1)
    with pytest.raises(ValueError, match="refine"):
        batch.run_batch([(A, b, c)], lockstep=True, workers=2, refine=1)
