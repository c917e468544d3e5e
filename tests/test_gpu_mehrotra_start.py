"""Mehrotra's starting point computed on the device (ipm_init_state_mehrotra, ipm_init_small_batch_mehrotra).

Yardstick: a dense float64 NumPy evaluation of the formulas (numpy_start below, restated here: unbounded as Mehrotra states them,
bounded as IpmSolver._mehrotra_start_bounded extends them).  Tolerance, per input and derived, not chosen: the relative error of the
host recipe IpmSolver.mehrotra_start() against NumPy on that input is measured first; the device start is allowed 10 x that error,
with a floor of 1e-13 (the two differ in summation order only; on the small path also in the order inside the factor).  Every
comparison input has full row rank (checked with np.linalg.matrix_rank when it is built), so no guarded pivot enters."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batch
from interiorpointmethod_amd.matio import load_npz_problem
from interiorpointmethod_amd.solver import IpmSolver, init_small_batch_mehrotra, solve_lockstep

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 1e-13


# ------------------------------------------------------------------------------------------- inputs and the yardstick
def numpy_start(A, b, c, u=None):
    """(x, y, s, w, z) by dense float64 NumPy; u = None or a length-n vector (+inf = none); w = z = 0 outside U."""
    Ad = A.toarray() if sparse.issparse(A) else np.asarray(A, dtype=np.float64)
    n = Ad.shape[1]
    u = np.full(n, np.inf) if u is None else np.asarray(u, dtype=np.float64)
    U = np.isfinite(u)
    G = Ad @ Ad.T
    x = Ad.T @ np.linalg.solve(G, b)
    y = np.linalg.solve(G, Ad @ c)
    r = c - Ad.T @ y
    w, z = np.zeros(n), np.zeros(n)
    w[U] = u[U] - x[U]
    s = r.copy()
    s[U] = np.maximum(r[U], 0.0)
    z[U] = np.maximum(-r[U], 0.0)
    dp = max(-1.5 * min(x.min(), w[U].min() if U.any() else np.inf), 0.0)
    dd = max(-1.5 * min(s.min(), z[U].min() if U.any() else np.inf), 0.0)
    x = x + dp; w[U] += dp
    s = s + dd; z[U] += dd
    xs = 0.5 * float(x @ s + w[U] @ z[U])
    pc = xs / float(s.sum() + z[U].sum())
    x = x + pc; w[U] += pc
    dc = xs / float(x.sum() + w[U].sum())
    s = s + dc; z[U] += dc
    return x, y, s, w, z


def random_lp(m, n, seed, dense=False):
    """Random A of full row rank (a scaled identity part plus sparse noise), b and c of mixed sign so that both shifts are at work."""
    rng = np.random.default_rng(seed)
    A = np.where(rng.random((m, n)) < min(1.0, 4.0 / m + 0.02), rng.standard_normal((m, n)), 0.0)
    A[np.arange(m), np.arange(m) % n] = 2.0 + rng.random(m)
    if m == 1:
        A[0, :] = [1.0, 2.0][:n] if n == 2 else A[0, :]
    assert np.linalg.matrix_rank(A) == m
    b = A @ rng.normal(0.5, 1.0, n)
    c = rng.standard_normal(n)
    return (A if dense else sparse.csc_matrix(A)), b, c


def netlib(name):
    A, b, c, cTlb, _ = load_npz_problem(os.path.join(GOLDEN, "netlib", name + ".npz"))
    return sparse.csc_matrix(A, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel(), float(cTlb)


def bounds(n, kind, seed=5):
    """kind: None / "empty" (all +inf) / "subset" (every third column) / "all"."""
    if kind is None:
        return None
    u = np.full(n, np.inf)
    rng = np.random.default_rng(seed)
    if kind == "subset":
        u[::3] = rng.uniform(0.5, 2.0, len(u[::3]))
    elif kind == "all":
        u[:] = rng.uniform(0.5, 2.0, n)
    return u


SMALL_SHAPES = [(1, 2), (16, 40), (17, 40), (128, 300), (20, 511), (20, 512), (20, 513)]
# name -> (builder of (A, b, c), IpmSolver keywords)
MULTI = {
    "sparse129x260": (lambda: random_lp(129, 260, 11), {}),
    "rcm300x640": (lambda: random_lp(300, 640, 12), {"reorder": "rcm"}),
    "SC205": (lambda: netlib("SC205")[:3], {}),
    "sparse_factor200x420": (lambda: random_lp(200, 420, 13), {"factor": "sparse"}),
    "dense64x160": (lambda: random_lp(64, 160, 14, dense=True), {}),
    "dense200x520": (lambda: random_lp(200, 520, 15, dense=True), {}),
}


@functools.lru_cache(maxsize=None)
def small_case(m, n):
    return random_lp(m, n, 100 * m + n)


@functools.lru_cache(maxsize=None)
def multi_case(name):
    A, b, c = MULTI[name][0]()
    assert np.linalg.matrix_rank(A.toarray() if sparse.issparse(A) else A) == A.shape[0]
    return A, b, c


def rel(a, ref):
    return float(np.max(np.abs(np.ravel(a) - np.ravel(ref))) / max(1e-300, float(np.max(np.abs(ref)))))


def device_state(sv):
    """(x, y, s, w, z) of the solver as flat arrays (w = z = 0 without bounds)."""
    x, y, s = (v.ravel() for v in sv.get_state())
    wz = sv.get_bound_state()
    w, z = (v.ravel() for v in wz) if wz is not None else (np.zeros(sv.n), np.zeros(sv.n))
    return x, y, s, w, z


def host_state(sv):
    out = [np.asarray(v, dtype=np.float64).ravel() for v in sv.mehrotra_start()]
    return tuple(out) if len(out) == 5 else tuple(out) + (np.zeros(sv.n), np.zeros(sv.n))


def check_against_numpy(A, b, c, u, what, **kw):
    """The derived-tolerance comparison of one input; returns the device state."""
    ref = numpy_start(A, b, c, u)
    with IpmSolver(A, b, c, ub=u, **kw) as sv:
        host = host_state(sv)
        nfix = sv.init_state_mehrotra()
        dev = device_state(sv)
    U = np.isfinite(u) if u is not None else np.zeros(len(c), dtype=bool)
    names = ("x", "y", "s") + (("w", "z") if U.any() else ())
    e_host = max(rel(h, r) for h, r, _ in zip(host, ref, names))
    e_dev = {k: rel(d, r) for d, r, k in zip(dev, ref, names)}
    tol = max(10.0 * e_host, FLOOR)
    print("[mehrotra-start] %-28s host %.3e  device %s  allowed %.3e" % (what, e_host, " ".join("%s=%.2e" % kv for kv in e_dev.items()), tol))
    assert nfix == 0, (what, nfix)
    assert max(e_dev.values()) <= tol, (what, e_dev, e_host, tol)
    x, y, s, w, z = dev
    assert x.min() > 0 and s.min() > 0, what
    if U.any():
        assert w[U].min() > 0 and z[U].min() > 0 and not w[~U].any() and not z[~U].any(), what
        # The recipe shifts x and w TOGETHER (w = u - x, then both += dp and += xs / ss), so x + w - u is not 0 but the same
        # 2 (dp + xs / ss) in every column of U: w = u - x, the two shifts of w and the two of x round once each
        ru = x[U] + w[U] - u[U]
        scale = max(np.max(np.abs(x)), np.max(np.abs(w)), np.max(u[U]))
        assert ru.max() - ru.min() <= 16 * np.finfo(float).eps * scale, (what, ru.min(), ru.max())
        assert abs(ru[0] - (ref[0][U] + ref[3][U] - u[U])[0]) <= 2 * tol * scale, what
    return dev


# ------------------------------------------------------------------------------------------- result
@pytest.mark.parametrize("kind", [None, "empty", "subset", "all"])
@pytest.mark.parametrize("m,n", SMALL_SHAPES)
def test_small_path_matches_numpy(m, n, kind):
    A, b, c = small_case(m, n)
    dev = check_against_numpy(A, b, c, bounds(n, kind), "small %dx%d %s" % (m, n, kind))
    if kind == "empty":                               # no finite bound: the plain start, bit for bit
        with IpmSolver(A, b, c) as sv:
            assert sv.schedule()["fused_small"] == 1
            sv.init_state_mehrotra()
            plain = device_state(sv)
        assert all(np.array_equal(p, d) for p, d in zip(plain, dev))


@pytest.mark.parametrize("kind", [None, "subset"])
@pytest.mark.parametrize("name", ["AFIRO", "SHARE1B"])
def test_small_path_netlib_matches_numpy(name, kind):
    A, b, c, _ = netlib(name)
    assert np.linalg.matrix_rank(A.toarray()) == A.shape[0]
    check_against_numpy(A, b, c, bounds(A.shape[1], kind), "small %s %s" % (name, kind))


@pytest.mark.parametrize("kind", [None, "subset"])
@pytest.mark.parametrize("name", sorted(MULTI))
def test_multi_kernel_path_matches_numpy(name, kind):
    A, b, c = multi_case(name)
    kw = MULTI[name][1]
    with IpmSolver(A, b, c, **kw) as sv:                  # the case runs the path it is named for
        assert sv.schedule()["fused_small"] == 0
        assert (sv.factor == "sparse") == (kw.get("factor") == "sparse")
        if kw.get("reorder") == "rcm" or sv.factor == "sparse":      # rows reordered (RCM / the sparse factor's own order): y must come back in the caller's
            assert sv._perm is not None and not np.array_equal(sv._perm, np.arange(sv.m))
        else:
            assert sv._perm is None
        assert sv.sparse == sparse.issparse(A)
    check_against_numpy(A, b, c, bounds(A.shape[1], kind), "multi %s %s" % (name, kind), **kw)


def test_lockstep_handle_matches_its_plain_twin():
    """An IPM_FLAG_LOCKSTEP handle (single stream, no group inverses skipped) starts within the same tolerance."""
    A, b, c = multi_case("sparse129x260")
    check_against_numpy(A, b, c, None, "lockstep sparse129x260", lockstep=True)


# ------------------------------------------------------------------------------------------- repeatability and handle state
def same(a, b):
    """Equality of statistics / history records, NaN == NaN."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    return np.array_equal(np.float64(a), np.float64(b), equal_nan=True)


def _bytes(sv):
    return b"".join(v.tobytes() for v in device_state(sv))


@pytest.mark.parametrize("which", ["small", "small_bounded", "sparse", "dense_bounded"])
def test_bitwise_repeat_and_handle_state(which):
    """Two starts on one handle give identical bytes; after a start the handle behaves as after init_state: solve() begins at
    iteration 0 with a fresh history, and start + solve a second time reproduces the first bit for bit."""
    if which.startswith("small"):
        A, b, c = small_case(17, 40)
        u = bounds(40, "subset") if which.endswith("bounded") else None
    elif which == "sparse":
        (A, b, c), u = multi_case("sparse129x260"), None
    else:
        (A, b, c), u = multi_case("dense64x160"), bounds(160, "subset")
    with IpmSolver(A, b, c, ub=u) as sv:
        sv.init_state_mehrotra()
        first = _bytes(sv)
        sv.init_state_mehrotra()
        assert _bytes(sv) == first
        st1 = dict(sv.solve(tol=1e-8, max_iter=7))
        h1, end1 = sv.history(), _bytes(sv)
        assert [r["k"] for r in h1] == list(range(st1["iterations"])) and st1["iterations"] > 0
        sv.init_state_mehrotra()
        assert _bytes(sv) == first
        st2 = dict(sv.solve(tol=1e-8, max_iter=7))
        st1.pop("solve_ms"); st2.pop("solve_ms")
        assert same(st2, st1) and same(sv.history(), h1) and _bytes(sv) == end1
        sv.init_state_mehrotra()                           # iterate() counts from 0 after a start, as after init_state
        assert sv.iterate(2)["iterations"] == 2 and [r["k"] for r in sv.history()] == [0, 1]


# ------------------------------------------------------------------------------------------- degenerate data
@pytest.mark.parametrize("which", ["small", "small_bounded", "sparse_bounded", "dense"])
def test_degenerate_data_gives_the_reference_start(which):
    """c = 0: y = 0 and s = 0, x.s = 0 -> exactly x = s = 1, y = 1 (w = z = 1 on U, 0 outside), what the host recipe returns."""
    if which.startswith("small"):
        A, b, _ = small_case(17, 40)
    elif which.startswith("sparse"):
        A, b, _ = multi_case("sparse129x260")
    else:
        A, b, _ = multi_case("dense64x160")
    n = A.shape[1]
    u = bounds(n, "subset") if which.endswith("bounded") else None
    with IpmSolver(A, b, np.zeros(n), ub=u) as sv:
        host = host_state(sv)
        sv.init_state_mehrotra()
        x, y, s, w, z = device_state(sv)
    U = np.isfinite(u) if u is not None else np.zeros(n, dtype=bool)
    assert np.array_equal(x, np.ones(n)) and np.array_equal(s, np.ones(n)) and np.array_equal(y, np.ones(A.shape[0]))
    assert np.array_equal(w, U.astype(float)) and np.array_equal(z, U.astype(float))
    for d, h in zip((x, y, s, w, z), host):
        assert np.array_equal(d, h)


# ------------------------------------------------------------------------------------------- pivot count
@pytest.mark.parametrize("m,n,kw", [(17, 40, {}), (129, 260, {}), (64, 160, {"dense": True})])
def test_pivots_fixed_counts_dependent_rows(m, n, kw):
    """(pivot_guard_eps = 1e-8: the pivot of a duplicated row is rounding noise of either sign around 0, far below 1e-8 max diag on
    every path, so the count does not depend on a summation order; the start uses the handle's guard as normal_solve does)"""
    kw = dict(kw, pivot_guard_eps=1e-8)
    A, b, c = random_lp(m, n, 77, dense="dense" in kw)
    Ad = A if "dense" in kw else A.toarray()
    dup = np.vstack([Ad, Ad[3:4]])                        # one duplicated row
    bd = np.concatenate([b, b[3:4]])
    for M, rhs, least in ((Ad, b, 0), (dup, bd, 1)):
        Ain = M if "dense" in kw else sparse.csc_matrix(M)
        with IpmSolver(Ain, rhs, c, **kw) as sv:
            sv.normal_solve(np.zeros(sv.m))
            want = sv.last_pivots_fixed
            got = sv.init_state_mehrotra()
        assert got == want == sv.last_pivots_fixed and (got >= 1 if least else got == 0), (m, n, got, want)


# ------------------------------------------------------------------------------------------- batch entry
def _mixed_batch():
    Ps = []
    for (m, n), kind in zip([(1, 2), (16, 40), (17, 40), (128, 300), (20, 513), (20, 511)], [None, "subset", None, "all", "subset", None]):
        A, b, c = small_case(m, n)
        Ps.append((A, b, c, bounds(n, kind)))
    A, b, c, _ = netlib("AFIRO")
    Ps.append((A, b, c, None))
    return Ps


def test_batch_entry_is_bit_identical_to_single_calls():
    Ps = _mixed_batch()
    svs = [IpmSolver(A, b, c, ub=u) for A, b, c, u in Ps]
    try:
        single, counts = [], []
        for sv in svs:
            counts.append(sv.init_state_mehrotra())
            single.append(_bytes(sv))
        for order in (list(range(len(svs))), list(range(len(svs)))[::-1], [3, 0, 5, 1, 6, 2, 4]):
            for sv in svs:
                sv.init_state(0.25)                       # something else in between
            got = init_small_batch_mehrotra([svs[i] for i in order])
            assert got == [counts[i] for i in order]
            for i in order:
                assert _bytes(svs[i]) == single[i], (order, i)
                assert svs[i].last_pivots_fixed == counts[i]
        # after the batch start every handle is ready to solve, from iteration 0
        st = ipm.solve_small_batch_solvers(svs, max_iter=3)
        assert all(r["iterations"] == 3 for r in st)
    finally:
        for sv in svs:
            sv.close()


def test_batch_entry_rejects_what_the_batch_solve_rejects():
    lib = _lib.load()
    Ps = _mixed_batch()
    a, b = (IpmSolver(A, bb, c, ub=u) for A, bb, c, u in Ps[1:3])
    big = IpmSolver(*multi_case("sparse129x260"))
    try:
        def call(svs, n=None):
            hs = (C.c_void_p * max(1, len(svs)))(*[sv._h if sv is not None else None for sv in svs])
            rc = lib.ipm_init_small_batch_mehrotra(hs, len(svs) if n is None else n, None, None)
            return rc, lib.ipm_last_error(None).decode()
        assert lib.ipm_init_small_batch_mehrotra(None, 0, None, None) == 0
        assert call([a], n=0)[0] == 0
        assert call([a], n=-1)[0] == -1
        assert lib.ipm_init_small_batch_mehrotra(None, 2, None, None) == -1
        rc, msg = call([a, None])
        assert rc == -1 and "handle 1 is NULL" in msg, msg
        rc, msg = call([a, big, b])
        assert rc == -1 and "handle 1 is not on the fused small-LP path" in msg, msg
        rc, msg = call([a, b, a])
        assert rc == -1 and "handle 2 is the same handle as handle 0" in msg, msg
        with pytest.raises(ValueError, match="solver 1"):
            init_small_batch_mehrotra([a, big])
        assert init_small_batch_mehrotra([]) == []
        assert lib.ipm_init_state_mehrotra(None, None) == -1
    finally:
        for sv in (a, b, big):
            sv.close()


# ------------------------------------------------------------------------------------------- end to end
SMALL_NETLIB = ["AFIRO", "ADLITTLE", "SHARE1B", "SC50A", "SC50B"]
# From the reference start x = s = 1 (max_iter = 300) two of the five do not converge, on the parent commit as here (that code is
# unchanged): ADLITTLE runs into the cap (status 2; DESIGN.md 4-M quotes it), SHARE1B ends in NaN (status 3; tests/test_gpu_small_batch.py)
NOT_CONVERGED_FROM_REFERENCE = {"ADLITTLE": 2, "SHARE1B": 3}


@pytest.fixture(scope="module")
def optima():
    return json.load(open(os.path.join(GOLDEN, "netlib_optima.json")))


def test_small_batch_end_to_end(optima):
    probs = [netlib(n) for n in SMALL_NETLIB]
    out = ipm.solve_small_batch([p[:3] for p in probs], tol=1e-8, max_iter=300, start="mehrotra")
    for name, (A, b, c, cTlb), (x, y, s, info) in zip(SMALL_NETLIB, probs, out):
        opt = optima[name]
        assert info["status"] == 1 and abs(info["objective"] - cTlb - opt) <= 1e-6 * max(1.0, abs(opt)), (name, info["status"], info["objective"])
        x1, y1, s1, one = ipm.solve_with_info(A, b, c, tol=1e-8, max_iter=300, start="mehrotra", device_start=True)
        assert np.array_equal(x, x1) and np.array_equal(y, y1) and np.array_equal(s, s1), name
        for k in ("status", "iterations", "objective", "rp_norm", "rd_norm", "gap", "pivots_fixed", "auto_regularized"):
            assert info[k] == one[k], (name, k)
    ref = ipm.solve_small_batch([probs[SMALL_NETLIB.index(n)][:3] for n in NOT_CONVERGED_FROM_REFERENCE], tol=1e-8, max_iter=300)
    for (name, status), (_, _, _, info) in zip(NOT_CONVERGED_FROM_REFERENCE.items(), ref):
        assert info["status"] == status, (name, info["status"])


def test_lockstep_end_to_end(optima):
    names = ["ISRAEL", "SCAGR25", "SC205"]
    probs = [netlib(n) for n in names]
    alone = []
    for A, b, c, _ in probs:
        with IpmSolver(A, b, c, lockstep=True, concurrent=True) as sv:
            sv.init_state_mehrotra()
            st = sv.solve(tol=1e-8, max_iter=300)
            alone.append((st["iterations"], _bytes(sv)))
    svs = [IpmSolver(A, b, c, lockstep=True, concurrent=True) for A, b, c, _ in probs]
    try:
        for sv in svs:
            sv.init_state_mehrotra()
        stats = solve_lockstep(svs, tol=1e-8, max_iter=300)
        for name, (A, b, c, cTlb), sv, st, (it, state) in zip(names, probs, svs, stats, alone):
            opt = optima[name]
            assert st["iterations"] == it and _bytes(sv) == state, name
            assert st["status"] == 1 and abs(st["objective"] - cTlb - opt) <= 1e-6 * max(1.0, abs(opt)), (name, st["status"])
    finally:
        for sv in svs:
            sv.close()
    P = [p[:3] for p in probs]
    rec, _ = batch.run_batch(P, workers=4, lockstep=True, tol=1e-8, max_iter=300, start="mehrotra")
    ref, _ = batch.run_batch(P, workers=4, lockstep=True, tol=1e-8, max_iter=300)
    assert [int(r[2]) for r in rec] == [it for it, _ in alone] and all(r[1] == 1.0 for r in rec)
    assert [int(r[2]) for r in rec] != [int(r[2]) for r in ref]
