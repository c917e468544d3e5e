"""GPU tests (-m gpu) of the pivot guard, the Tikhonov shift and the automatic 5 % shift on every dense Cholesky path:
the serial blocked factor (solve_linear; iterate with IPM_FUSED_FACTOR=0, its look-ahead, two-level and bulk-update
variants), the fused formation + factor (IPM_FUSED_FACTOR=force and the default at 16 blocks), the lockstep batch and the
fused small-LP kernel.  The matrices come from guard_cases.py: every guarded pivot is exactly 0.0 and the guarded factor is
known in closed form, so the guard count, the guarded positions and the unguarded part of L are asserted EXACTLY."""
import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                                                # noqa: E402
from guard_cases import BIG, EPS, GuardCase, auto_shift_boundary, guard_rows         # noqa: E402

U = 2.0 ** -53
SIGMA = 2.0 ** -20            # the explicit shift of (c): no pivot is guarded under it


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _rhs(m, seed=0):
    return np.random.default_rng(seed + m).standard_normal(m)


def check_factor(L, c, k=0, where=""):
    """(a): unguarded columns equal the closed form bitwise (the t+ row's sqrt to 2 ulp), guarded diagonals sqrt(big) to
    2 ulp, guarded off-diagonals below 2^-90 max|B|."""
    E = c.expected_factor(k)
    Lc = L.copy()
    for r in c.inexact_diag():
        assert abs(L[r, r] - E[r, r]) <= 2 * np.spacing(E[r, r]), (where, r, L[r, r], E[r, r])
        Lc[r, r] = E[r, r]
    keep, g = c.keep, np.array(c.guarded, dtype=np.int64)
    bad = np.argwhere(Lc[:, keep] != E[:, keep])
    assert bad.size == 0, (where, [(int(i), int(keep[j]), Lc[i, keep[j]], E[i, keep[j]]) for i, j in bad[:5]])
    if g.size:
        dg = np.diag(L)[g]
        assert np.all(np.abs(dg - np.sqrt(BIG)) <= 2 * np.spacing(np.sqrt(BIG))), (where, g[np.abs(dg - np.sqrt(BIG)) > 0][:5])
        off = np.tril(L, -1)[:, g]
        assert np.max(np.abs(off)) <= 2.0 ** -90 * c.maxdiag * 4.0 ** k, (where, np.max(np.abs(off)))


def check_solution(z, c, B, rhs, where=""):
    z = np.asarray(z).ravel()
    zr = c.reduced_solution(B, rhs)
    keep = c.keep
    # componentwise: the t+ row's 1/(eps maxdiag) would hide every other row's error in a max-norm bound
    plain = np.array([j for j in keep if j not in c.decoupled], dtype=np.int64)
    scale = np.max(np.abs(zr[plain])) if plain.size else 0.0
    err = np.abs(z[keep] - zr[keep])
    assert np.all(err <= 1e-10 * (np.abs(zr[keep]) + scale)), (where, keep[np.argmax(err)], float(np.max(err)))
    if c.guarded:
        assert np.max(np.abs(z[c.guarded])) <= 1e-60 * np.linalg.norm(rhs), where


def check_shift(L, B, maxdiag, sigma, m, where=""):
    """(c): diag(L L^T - B) = sigma max diag(B) on every true row; backward error of B + sigma max diag(B) I."""
    shift = sigma * maxdiag
    Ll = L.astype(np.longdouble)
    d = np.sum(Ll * Ll, axis=1) - np.diag(B).astype(np.longdouble)
    assert np.all(np.abs(d - shift) <= 1e-12 * maxdiag), (where, np.flatnonzero(np.abs(d - shift) > 1e-12 * maxdiag)[:8])
    R = L @ L.T - (B + shift * np.eye(m))
    assert np.max(np.abs(R)) <= 64 * m * U * np.max(np.abs(B)), (where, np.max(np.abs(R)))


def _linear(m, **opts):
    return ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1), **opts)


# ------------------------------------------------------------------ solve_linear: the serial blocked factor
LINEAR = [(m, {}) for m in (1, 17, 128, 129, 300, 1100, 2100, 2500)] + \
         [(1100, {"IPM_GROUP_STEPS": "2"}), (1100, {"IPM_LOOKAHEAD": "0"}), (2100, {"IPM_GROUPED_TRSV": "0"})]


@pytest.mark.parametrize("m,env", LINEAR)
def test_solve_linear_guard_is_exact(m, env, monkeypatch):
    _env(monkeypatch, env)
    c = GuardCase(m, boundary=m >= 17, negative=m >= 17)
    B, rhs = c.B(), _rhs(m)
    with _linear(m) as sv:
        z, nfix = sv.solve_linear(B, rhs)
        L = sv.get_factor()
    assert nfix == len(c.guarded)
    check_factor(L, c, where=(m, env))
    check_solution(z, c, B, rhs, where=(m, env))


@pytest.mark.parametrize("m", [129, 1100])
@pytest.mark.parametrize("eps", [EPS, 2.0 ** -60])
def test_solve_linear_threshold_boundary(m, eps):
    """(b): eps * maxdiag itself and the value one ulp below it are guarded, the value one ulp above it is not; -1 is guarded
    and leaves the max alone; a NaN diagonal never wins the max and is guarded, the other rows do not notice it."""
    c = GuardCase(m, boundary=True, negative=True, eps=eps, seed=11)
    B, rhs = c.B(), _rhs(m, 1)
    plain = [j for j in c.keep if j not in c.decoupled and not np.any(c.N[j]) and not np.any(c.N[:, j])]
    jn = int(plain[len(plain) // 2])
    B[jn, jn] = np.nan
    c.guarded = sorted(c.guarded + [jn])
    c.keep = np.array([j for j in c.keep if j != jn], dtype=np.int64)
    with _linear(m, pivot_guard_eps=eps) as sv:
        z, nfix = sv.solve_linear(B, rhs)
        L = sv.get_factor()
    assert nfix == len(c.guarded)
    check_factor(L, c, where=(m, eps))
    Bk = B.copy()
    Bk[jn, jn] = 0.0
    check_solution(z, c, Bk, rhs, where=(m, eps))


@pytest.mark.parametrize("m", [129, 300, 1100])
def test_solve_linear_shift_reaches_every_diagonal(m):
    c = GuardCase(m, boundary=True, seed=3)
    B = c.B()
    with _linear(m, regularize=SIGMA) as sv:
        _, nfix = sv.solve_linear(B, _rhs(m))
        L = sv.get_factor()
    assert nfix == 0
    check_shift(L, B, c.maxdiag, SIGMA, m, where=m)


@pytest.mark.parametrize("m", [129, 1100])
def test_solve_linear_scale_invariance(m):
    """(d): d scaled by 4^k: the same guard decisions, the unguarded part of L scaled by exactly 2^k."""
    c = GuardCase(m, boundary=True, negative=True, seed=4)
    for k in (-150, -70, 70):
        B = c.B(4.0 ** k)
        with _linear(m) as sv:
            _, nfix = sv.solve_linear(B, _rhs(m))
            L = sv.get_factor()
        assert nfix == len(c.guarded), k
        check_factor(L, c, k=k, where=(m, k))


# ------------------------------------------------------------------ iterate: the serial and the fused factor of A diag(d) A^T
def _lp(c, as_sparse=False):
    A = sparse.csc_matrix(c.A) if as_sparse else c.A
    return A, c.A @ np.ones(c.n), np.ones(c.n)


def _iterate(c, scale=1.0, **opts):
    A, b, cv = _lp(c)
    with ipm.IpmSolver(A, b, cv, reorder=None, factor="dense", auto_regularize=False, **opts) as sv:
        assert sv._perm is None
        x, s = c.x_state(scale)
        sv.set_state(x, np.zeros(c.m), s)
        st = sv.iterate(1)
        return st, sv.get_factor(), sv.history(), sv.schedule()


ITERATE = [(m, {"IPM_FUSED_FACTOR": f}) for m in (400, 1100, 2100) for f in ("0", "force")] + \
          [(1100, {"IPM_FUSED_FACTOR": "0", "IPM_BULK_VARIANT": v}) for v in ("0", "7")]


@pytest.mark.parametrize("m,env", ITERATE + [(2048, {})])
def test_iterate_guard_is_exact(m, env, monkeypatch):
    _env(monkeypatch, env)
    c = GuardCase(m, boundary=True, negative=True, seed=7)
    st, L, hist, sched = _iterate(c)
    if not env:
        assert sched["fused_factor"] == 1                    # the default rule at 16 blocks
    elif env.get("IPM_FUSED_FACTOR") == "0":
        assert sched["fused_factor"] == 0
    assert st["pivots_fixed"] == len(c.guarded) and hist[0]["pivots_fixed"] == len(c.guarded)
    check_factor(L, c, where=(m, env))


@pytest.mark.parametrize("fused", ["0", "force"])
@pytest.mark.parametrize("eps", [EPS, 2.0 ** -60])
def test_iterate_threshold_boundary(fused, eps, monkeypatch):
    monkeypatch.setenv("IPM_FUSED_FACTOR", fused)
    c = GuardCase(1100, boundary=True, negative=True, eps=eps, seed=12)
    st, L, _, _ = _iterate(c, pivot_guard_eps=eps)
    assert st["pivots_fixed"] == len(c.guarded)
    check_factor(L, c, where=(fused, eps))


@pytest.mark.parametrize("m", [400, 1100])
@pytest.mark.parametrize("fused", ["0", "force"])
def test_iterate_shift_reaches_every_diagonal(m, fused, monkeypatch):
    monkeypatch.setenv("IPM_FUSED_FACTOR", fused)
    c = GuardCase(m, boundary=True, seed=8)
    st, L, _, _ = _iterate(c, regularize=SIGMA)
    assert st["pivots_fixed"] == 0
    check_shift(L, c.B(), c.maxdiag, SIGMA, m, where=(m, fused))


@pytest.mark.parametrize("fused", ["0", "force"])
def test_iterate_scale_invariance(fused, monkeypatch):
    monkeypatch.setenv("IPM_FUSED_FACTOR", fused)
    c = GuardCase(1100, boundary=True, negative=True, seed=9)
    for k in (-150, -70, 70):
        st, L, _, _ = _iterate(c, scale=4.0 ** k)
        assert st["pivots_fixed"] == len(c.guarded), k
        check_factor(L, c, k=k, where=(fused, k))


# ------------------------------------------------------------------ the lockstep batch
def _lockstep_handle(c, scale=1.0, **opts):
    A, b, cv = _lp(c, as_sparse=True)
    sv = ipm.IpmSolver(A, b, cv, lockstep=True, factor="dense", reorder=None, **opts)
    assert sv._perm is None and ipm.lockstep_eligible(sv)
    x, s = c.x_state(scale)
    sv.set_state(x, np.zeros(c.m), s)
    return sv


def _alone(c, scale=1.0, max_iter=1, **opts):
    with _lockstep_handle(c, scale, **opts) as sv:
        st = sv.solve(max_iter=max_iter)
        return st, sv.get_state()


@pytest.mark.parametrize("variant", ["exact", "shift", "scale-70", "scale-150", "eps2^-60"])
def test_lockstep_guard_is_exact(variant):
    """(a)-(d) on a batch of three LPs (2, 3 and 6 blocks): counts and factors exact, and every LP of the batch bit-identical
    to the same handle solved alone."""
    eps = 2.0 ** -60 if variant == "eps2^-60" else EPS
    opts = dict(auto_regularize=False, pivot_guard_eps=eps)
    k = {"scale-70": -70, "scale-150": -150}.get(variant, 0)
    if variant == "shift":
        opts["regularize"] = SIGMA
    cases = [GuardCase(m, boundary=True, negative=variant != "shift", eps=eps, seed=20 + m) for m in (129, 300, 700)]
    ref = [_alone(c, 4.0 ** k, **opts) for c in cases]
    svs = [_lockstep_handle(c, 4.0 ** k, **opts) for c in cases]
    try:
        stats = ipm.solve_lockstep(svs, max_iter=1)
        for c, sv, st, (st0, state0) in zip(cases, svs, stats, ref):
            want = 0 if variant == "shift" else len(c.guarded)
            assert st["pivots_fixed"] == want and st0["pivots_fixed"] == want, (c.m, st["pivots_fixed"], st0["pivots_fixed"])
            for a0, a1 in zip(sv.get_state(), state0):
                assert np.array_equal(a0, a1, equal_nan=True), c.m
            L = sv.get_factor()
            if variant == "shift":
                check_shift(L, c.B(), c.maxdiag, SIGMA, c.m, where=("lockstep", c.m))
            else:
                check_factor(L, c, k=k, where=("lockstep", c.m, variant))
    finally:
        for sv in svs:
            sv.close()


# ------------------------------------------------------------------ the fused small-LP kernel (m <= 128)
def _small(c, scale=1.0, **opts):
    A, b, cv = _lp(c, as_sparse=True)
    with ipm.IpmSolver(A, b, cv, factor="dense", reorder=None, **opts) as sv:
        fused = sv.schedule()["fused_small"]
        x, s = c.x_state(scale)
        sv.set_state(x, np.zeros(c.m), s)
        st = sv.solve(max_iter=1)
        return fused, st, sv.history(), sv.get_state()


@pytest.mark.parametrize("m", [27, 120])
@pytest.mark.parametrize("variant", ["exact", "eps2^-60", "shift", "scale-150", "scale-70", "scale70"])
def test_small_lp_guard(m, variant, monkeypatch):
    """The guard count of the first factorization exact, and the first iterate equal to the multi-kernel path's
    (IPM_FUSED_SMALL=0) to the bound of test_fused_small_lp_path: a shift missing from the small-LP site, or a guard
    decision that differs, moves it far beyond that."""
    eps = 2.0 ** -60 if variant == "eps2^-60" else EPS
    k = {"scale-150": -150, "scale-70": -70, "scale70": 70}.get(variant, 0)
    opts = dict(auto_regularize=False, pivot_guard_eps=eps)
    if variant == "shift":
        opts["regularize"] = SIGMA
    c = GuardCase(m, boundary=True, eps=eps, seed=30)
    fused, st, hist, state = _small(c, 4.0 ** k, **opts)
    assert fused == 1
    want = 0 if variant == "shift" else len(c.guarded)
    assert hist[0]["pivots_fixed"] == want and st["pivots_fixed"] == want
    monkeypatch.setenv("IPM_FUSED_SMALL", "0")
    fused0, st0, hist0, state0 = _small(c, 4.0 ** k, **opts)
    assert fused0 == 0 and hist0[0]["pivots_fixed"] == want
    for a, a0 in zip(state, state0):
        assert np.all(np.isfinite(a))
        assert np.max(np.abs(a - a0)) <= 1e-9 * max(1e-300, np.max(np.abs(a0))), variant


# ------------------------------------------------------------------ (e) the automatic 5 % shift, at its boundary
def _five_pct_case(m, k):
    rows = guard_rows(m)
    rows = rows + [r for r in range(m) if r not in rows]
    return GuardCase(m, guarded=rows[:k], seed=40 + k, coupled_frac=0.1)


def _check_auto(k, st, hist, st_off, hist_off, kb, where):
    if k == kb:
        assert st["auto_regularized"] == 0 and hist[0]["pivots_fixed"] == k, (where, st["auto_regularized"], hist[0])
    else:
        assert st["auto_regularized"] == 1, where
        assert hist[0]["pivots_fixed"] == 0, where                        # the restart runs under the 1e-14 shift
    assert st_off["auto_regularized"] == 0 and hist_off[0]["pivots_fixed"] == k, where


def _solve2(c, as_sparse, **opts):
    A, b, cv = _lp(c, as_sparse)
    with ipm.IpmSolver(A, b, cv, factor="dense", reorder=None, **opts) as sv:
        x, s = c.x_state()
        sv.set_state(x, np.zeros(c.m), s)
        st = sv.solve(max_iter=2)
        return st, sv.history(), sv.schedule()["fused_small"]


@pytest.mark.parametrize("m,as_sparse,small", [(200, False, 0), (120, True, 1)])
def test_auto_shift_five_percent_boundary(m, as_sparse, small):
    kb = auto_shift_boundary(m)
    for k in (kb, kb + 1):
        c = _five_pct_case(m, k)
        assert len(c.guarded) == k
        st, hist, fs = _solve2(c, as_sparse)
        st_off, hist_off, _ = _solve2(c, as_sparse, auto_regularize=False)
        assert fs == small
        _check_auto(k, st, hist, st_off, hist_off, kb, (m, k))


def test_auto_shift_five_percent_boundary_lockstep():
    """The batch's own copy of the rule (ipm_batch_step): the LP at k + 1 restarts with the shift, its neighbours -- the
    one at k and a full-rank one -- run on without it."""
    m = 200
    kb = auto_shift_boundary(m)
    cases = [_five_pct_case(m, kb), _five_pct_case(m, kb + 1), GuardCase(300, guarded=[], seed=50)]
    svs = [_lockstep_handle(c) for c in cases]
    try:
        stats = ipm.solve_lockstep(svs, max_iter=2)
        hists = [sv.history() for sv in svs]
    finally:
        for sv in svs:
            sv.close()
    assert [st["auto_regularized"] for st in stats] == [0, 1, 0]
    assert hists[0][0]["pivots_fixed"] == kb and hists[1][0]["pivots_fixed"] == 0 and hists[2][0]["pivots_fixed"] == 0
    off = [_alone(c, max_iter=2, auto_regularize=False)[0] for c in cases[:2]]
    assert [st["auto_regularized"] for st in off] == [0, 0]
