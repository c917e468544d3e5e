"""A solve must not depend on how far the host runs ahead of its stop test.

ipm_solve enqueues check_every iterations at a time and reads the scalar record once per chunk (csrc/ipm_api.hip, csrc/host_iteration.h);
the launches behind a satisfied stop test return at entry.  A solve that reports K iterations had its stop test fire in the (K + 1)-th
enqueued iteration, so with check_every = c the host enqueued c ceil((K + 1) / c) iterations and

    D = c ceil((K + 1) / c) - (K + 1)

whole dead iterations follow the firing one (plus the dead remainder of the firing iteration itself).  The rest of the suite runs
every solve with c = 4; here c is the controlled variable.  Every cell computes D for each c it runs, prints the (c, K, D) table and
the schedule words it asserted, and asserts that its c values realise D = 0, D = 1, some D >= 2 and D = c - 1 for some c >= 3.

A run (_record), on a fresh handle with check_every = c, everything collected as bytes (Obs of test_gpu_residue.py):
  1. the start, solve(tol, max_iter): statistics without solve_ms, state and bound state, history, corrector_info (correctors on),
     certificate (status 5 / 6), get_factor (dense-tile handles; not after K = 0 off the overlap path, where no factorization has
     run and B is memory nobody wrote), factor_info (sparse-factor handles; serial_launches must be 0: no time-out was recovered);
  2. on the same handle, no new state, iterate(1): statistics, state, history, the factor -- the continuation behind the dead tail;
  3. on the same handle, the start again and solve(max_iter=2): statistics, state, history -- a stale epoch, counter, hand-off word,
     latch or history index left by dead launches shows here.
schedule()["timeouts_recovered"] == 0 at the end.

Asserted: (a) chunk invariance -- the records of all c of a cell equal the record of c = 1, byte for byte; (b) an oracle that never
runs ahead -- a fresh handle, the same start, iterate(K) (exactly K live iterations, then the residuals) has the solve's (x, y, s, w,
z), history and statistics (but the status) byte for byte: a kernel that forgets `done` but computes the same from the same stale
input for every D >= 0 is invisible between the chunk lengths and shows here; for K = 0 the state is init_state's own (x = s = 1,
y = y0, w = z = 1 on the bounded set), status 2, iterations 0, empty history; (c) the path -- schedule() / factor_info() words of
the cell.  The factor is compared between c values only: after a stop the overlap path holds the factor of iterate K (its formation
tests the latch Scalars::done_f, taken before the concurrent stop test fires), the other paths and iterate(K) that of iterate K - 1.

Cap-stopped cells: K = 3 with c in {1, 2, 3, 4, 5, 7} (D = 0, 0, 2, 0, 1, 3) and K = 0, K = 2 with c = 4 (D = 3, 1; with K = 0
every launch of the solve is dead), each against c = 1 at the same K.  The cells that stop by another branch of the stop test run
c in {1, 2, 3, 4, 5, 7} at whatever K results.

FIGURES of the first run on an MI355X (K, then D for c = 1, 2, 3, 4, 5, 7):
  convergence   dense 2 blocks      tol 1e-8   K = 15   D = 0 0 2 0 4 5
                sparse A 130 x 257  tol 1e-8   K = 16   D = 0 1 1 3 3 4
                dense 9 blocks      tol 1e-7   K = 18   D = 0 1 2 1 1 2     (tol 1e-8: K = 19, D = 0 0 1 0 0 1, one nonzero value)
                overlap 16 blocks   tol 1e-7   K = 18   D = 0 1 2 1 1 2     (tol 1e-8: K = 19, the same)
  detection     primal_dense        status 5   K =  9   D = 0 0 2 2 0 4
                dual_dense          status 6   K =  8   D = 0 1 0 3 1 5
  NaN           x1 + x2 = -1        status 3   K = 25   D = 0 0 1 2 4 2
  automatic shift, lockstep batch and every cap-stopped cell: K as set.
Every record was equal between the chunk lengths and every iterate equal to iterate(K)'s: no cell narrowed.  Cells dropped: none.

FOUND with it (test_overlap_factor_solves_after_a_stop, the one observable of a stop that the record above cannot hold, because
ipm_normal_solve restarts the iteration count): on the overlap path the inverses of the last diagonal group tested `done` where the
factorization in front of them tests the latch, so after ANY stop (D = 0 included) the handle held the factor of iterate K with the
last group's inverses of iterate K - 1, and normal_solve(reuse_factor=True) answered with a relative error of 0.32 (fused launch)
and 5.3e-3 (serial factorization) at K = 3.  enqueue_iteration now gives the group inverses and their gate the latch: 2.2e-13 against
a bound of 3.3e-4 (fused), the same bytes (serial).

SENSITIVITY, checked once by hand on two libraries with one `done` test taken out.  corrector_rhs_kernel: all ten cells it was run
on fail at solve.stats.sigma against iterate(K) -- and only there: the kernel computes the same from the same stale input in the
firing iteration and in every dead one, so the chunk lengths agree with each other.  mu_aff_kernel: every cell passes, rightly; with
its neighbours dead the kernel rewrites, from unchanged partials, the values it wrote when it was live.

The file runs in 12 seconds on an MI355X (33 tests, the longest under 2 seconds).
"""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib
from interiorpointmethod_amd.workloads import synthetic_lp

import infeas_cases as IC
import iteration_oracle as IO
import sparse_cases as SC
import test_gpu_pivot_guard as PG
from guard_cases import auto_shift_boundary
from test_gpu_residue import SP_ENV, Obs, _block_bidiagonal, _feasible, _half_bounded

pytestmark = pytest.mark.gpu

Y0 = 1.0
CS = (1, 2, 3, 4, 5, 7)
CAP_RUNS = tuple((c, 3) for c in CS) + ((1, 0), (4, 0), (1, 2), (4, 2))          # (check_every, max_iter = K)
CLEARED = ("IPM_CHECK_EVERY", "IPM_TEST_ALLOC_FILL", "IPM_FUSED_SMALL", "IPM_FUSED_FACTOR", "IPM_STREAM_AT", "IPM_FLAG_SYNC",
           "IPM_GROUPED_TRSV", "IPM_GROUP_STEPS", "IPM_LIST_FORM", "IPM_ENVELOPE") + SP_ENV


def dead(c, K):
    """Whole dead iterations behind the firing one: the solve reported K iterations under check_every = c."""
    return c * -(-(K + 1) // c) - (K + 1)


def _covers_every_tail(runs):
    """The (c, K) of a cap-stopped cell realise D = 0, D = 1, some D >= 2 and D = c - 1 for some c >= 3."""
    ds = [(c, dead(c, K)) for c, K in runs]
    assert any(d == 0 for _, d in ds) and any(d == 1 for _, d in ds) and any(d >= 2 for _, d in ds), ds
    assert any(d == c - 1 and c >= 3 for c, d in ds), ds


# ---- one run ---------------------------------------------------------------------------------------------------------------
def _start(sv):
    sv.init_state(Y0)


def _record(make, c, max_iter, tol=1e-8, start=_start, overlap=False, check=None):
    """The three steps of the module docstring on make(c) -> (Obs, status, K)."""
    o = Obs()
    with make(c) as sv:
        dense_B = sv.factor == "dense" and not sv.schedule()["fused_small"]
        start(sv)
        st = sv.solve(tol=tol, max_iter=max_iter)
        K = st["iterations"]
        o.put("solve.stats", st)
        o.put("solve.state", sv.get_state())
        o.put("solve.bound_state", sv.get_bound_state())
        o.put("solve.history", sv.history())
        if sv.correctors:
            o.put("solve.correctors", sv.corrector_info())
        if st["status"] in (5, 6):
            o.put("solve.certificate", sv.certificate())
        if dense_B and (K > 0 or overlap):
            o.put("solve.L", sv.get_factor())
        if sv.factor == "sparse":
            fi = sv.factor_info()
            assert fi["serial_launches"] == 0, fi
            o.put("solve.factor_info", fi)
        assert sv.schedule()["timeouts_recovered"] == 0
        words = check(sv) if check else {}
        o.put("iterate1.stats", sv.iterate(1))                      # behind the dead tail, from the stopped iterate
        o.put("iterate1.state", sv.get_state())
        o.put("iterate1.bound_state", sv.get_bound_state())
        o.put("iterate1.history", sv.history())
        if sv.correctors:
            o.put("iterate1.correctors", sv.corrector_info())
        if dense_B:
            o.put("iterate1.L", sv.get_factor())
        start(sv)
        o.put("again.stats", sv.solve(tol=tol, max_iter=2))
        o.put("again.state", sv.get_state())
        o.put("again.bound_state", sv.get_bound_state())
        o.put("again.history", sv.history())
        if sv.correctors:
            o.put("again.correctors", sv.corrector_info())
        sch = sv.schedule()
        assert sch["timeouts_recovered"] == 0 and sch["live_handles"] == 1, sch
    return o, st["status"], K, words


def _oracle(make, K, start=_start):
    """K live iterations and nothing behind them but the final residuals: statistics, (x, y, s), (w, z) and history as bytes."""
    o = Obs()
    with make(1) as sv:
        start(sv)
        st = sv.iterate(K)
        assert st["iterations"] == K, st
        o.put("solve.stats", st)
        o.put("solve.state", sv.get_state())
        o.put("solve.bound_state", sv.get_bound_state())
        o.put("solve.history", sv.history())
        o.shape = sv.m, sv.n
    return o


def _first_difference(ref, got):
    """Names of the observables that differ, in the order they were recorded."""
    assert list(ref.bytes) == list(got.bytes), (sorted(set(ref.bytes) ^ set(got.bytes)))
    return [k for k in ref.bytes if ref.bytes[k] != got.bytes[k]]


def _init_state_values(o, ub, m, n):
    """K = 0: the state is init_state's own."""
    x, y, s = (np.frombuffer(o.bytes["solve.state[%d]" % i]) for i in range(3))
    assert x.shape == (n,) and y.shape == (m,) and np.all(x == 1.0) and np.all(s == 1.0) and np.all(y == Y0)
    if ub is not None and np.isfinite(ub).any():
        w, z = (np.frombuffer(o.bytes["solve.bound_state[%d]" % i]) for i in range(2))
        U = np.isfinite(ub)
        assert np.all(w[U] == 1.0) and np.all(z[U] == 1.0) and not np.any(w[~U]) and not np.any(z[~U])
    assert o.bytes["solve.history.len"] == b"0" and o.bytes["solve.stats.status"] == b"2" and o.bytes["solve.stats.iterations"] == b"0"


def _cell(monkeypatch, name, make, env=None, runs=CAP_RUNS, max_iter=None, status=2, oracle=True, check=None, overlap=False,
          ub=None, start=_start, tol=1e-8, tails=True):
    """runs: (c, K) pairs, cap-stopped at max_iter = K; with max_iter given, the c values of runs stop by another branch of the stop
    test (`status`) at whatever K results.  -> {c: K} of the runs at the largest cap, for the callers that assert on it."""
    with monkeypatch.context() as mp:
        for k in CLEARED:
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        base, got, words = {}, [], None
        for c, cap in sorted(runs, key=lambda r: (r[1], r[0])):               # c = 1 first at every cap
            o, stat, K, words = _record(make, c, cap if max_iter is None else max_iter, tol=tol, start=start, overlap=overlap, check=check)
            assert stat == status and (max_iter is not None or K == cap), (name, c, cap, stat, K)
            print("RUN-AHEAD %s: c = %d  K = %d  D = %d  status %d" % (name, c, K, dead(c, K), stat))
            got.append((c, K))
            if c == 1:
                base[cap] = o, K
                if oracle:
                    orc = _oracle(make, K, start)
                    differ = _first_difference(_oracle_view(orc, overlap), _oracle_view(o, overlap))
                    assert not differ, (name, "iterate(%d) against the solve" % K, differ)
                    if K == 0 and start is _start:
                        _init_state_values(o, ub, *orc.shape)
                continue
            ref, K1 = base[cap]
            assert K == K1, (name, c, K, K1)
            differ = _first_difference(ref, o)
            assert not differ, (name, "c = %d against c = 1 at K = %d, D = %d" % (c, K, dead(c, K)), differ)
        print("RUN-AHEAD %s: path words %s" % (name, words))
        if tails:
            _covers_every_tail(got)
        return got


def _oracle_view(o, overlap):
    """What a solve that stopped after K iterations shares with iterate(K): the iterate, the history, and the statistics but for the
    status (ipm_iterate takes no stop decision) and, on the overlap path, the guarded pivots (of the factor of iterate K there, of
    iterate K - 1 after ipm_iterate)."""
    skip = ("solve.stats.status",) + (("solve.stats.pivots_fixed",) if overlap else ())
    s = Obs()
    keep = ("solve.state", "solve.bound_state", "solve.history", "solve.stats")
    s.bytes = {k: v for k, v in o.bytes.items() if k.startswith(keep) and k not in skip}
    return s


def _words(sv, **want):
    """The schedule words a cell asserts -> what it asserted, for the print."""
    sch = sv.schedule()
    assert {k: sch[k] for k in want} == want, sch
    return want


# ---- the LPs (built once, never written to) --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _syn(m, n, seed):
    return synthetic_lp(m, n, seed=seed)


@functools.lru_cache(maxsize=None)
def _sparse130():
    A, b, c, ub = _feasible(IO.get("sparse/" + IO.shape_name(*IO.SMALL, True)))
    return sparse.csc_matrix(A), b, c, ub


@functools.lru_cache(maxsize=None)
def _sparsified(m, n, seed, density):
    """synthetic_lp's shape made sparse: the entries under a random mask, no empty row or column, a strictly feasible pair."""
    rng = np.random.default_rng(seed)
    A = synthetic_lp(m, n, seed=seed)[0] * (rng.random((m, n)) < density)
    A[np.arange(m), rng.integers(0, n, m)] = 1.0 + rng.random(m)
    A[rng.integers(0, m, n), np.arange(n)] += 1.0 + rng.random(n)
    x0, y0, s0 = rng.uniform(0.5, 1.5, n), rng.standard_normal(m), rng.uniform(0.5, 1.5, n)
    return sparse.csc_matrix(A), A @ x0, A.T @ y0 + s0


# ---- cells that stop at the cap --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "half-bounded"])
def test_dense_two_blocks(monkeypatch, bounded):
    """130 x 257 dense: two blocks, one stream, everything tests Scalars::done."""
    A, b, c = _syn(130, 257, 11)
    ub = _half_bounded(257) if bounded else None

    def check(sv):
        assert not sv.sparse and sv.bounded == (129 if bounded else 0)
        return _words(sv, blocks=2, fused_factor=0, fused_small=0, grouped_trsv=1, device_polling=0)
    _cell(monkeypatch, "dense-2-blocks" + ("-bounded" if bounded else ""), lambda ce: ipm.IpmSolver(A, b, c, ub=ub, check_every=ce),
          check=check, ub=ub)


NINE = {"default": ({}, dict(device_polling=1, grouped_trsv=1, group_steps=1)),
        "events": ({"IPM_FLAG_SYNC": "0"}, dict(device_polling=0, grouped_trsv=1, group_steps=1)),
        "block-steps": ({"IPM_GROUPED_TRSV": "0"}, dict(device_polling=1, grouped_trsv=0, group_steps=1)),
        "two-level": ({"IPM_GROUP_STEPS": "2"}, dict(device_polling=1, grouped_trsv=1, group_steps=2))}


@pytest.mark.parametrize("variant", sorted(NINE))
def test_dense_nine_blocks(monkeypatch, variant):
    """1100 x 1400: the polled look-ahead Cholesky on the bulk stream (d_bulk_done, events recorded for dead factorizations), one group
    of 8 and a leftover block; with stream events instead of polling; block steps; two-level steps."""
    env, want = NINE[variant]
    A, b, c = _syn(1100, 1400, 12)
    _cell(monkeypatch, "dense-9-blocks-" + variant, lambda ce: ipm.IpmSolver(A, b, c, check_every=ce), env=env,
          check=lambda sv: _words(sv, blocks=9, fused_factor=0, fused_small=0, **want))


def test_fused_three_blocks(monkeypatch):
    """300 x 600 under IPM_FUSED_FACTOR=force: the fused formation + factorization launch below the overlap path (it tests done)."""
    A, b, c = _syn(300, 600, 13)
    _cell(monkeypatch, "fused-3-blocks", lambda ce: ipm.IpmSolver(A, b, c, check_every=ce), env={"IPM_FUSED_FACTOR": "force"},
          check=lambda sv: _words(sv, blocks=3, fused_factor=1, device_polling=1, fused_small=0))


OVERLAP = {"default": ({}, dict(fused_factor=1, stream_at=1)),
           "serial": ({"IPM_FUSED_FACTOR": "0"}, dict(fused_factor=0, stream_at=1)),
           "unstreamed": ({"IPM_STREAM_AT": "0"}, dict(fused_factor=1, stream_at=0))}


def test_overlap_cells_run_fused_and_serial():
    assert {w["fused_factor"] for _, w in OVERLAP.values()} == {0, 1}           # (each cell asserts its word from schedule())


@pytest.mark.parametrize("variant", sorted(OVERLAP))
def test_overlap_sixteen_blocks(monkeypatch, variant):
    """2048 x 2500: the residual stream.  Formation and factorization test the latch done_f that scaling_kernel took while the stop
    test of the same iterate runs concurrently; the last group's inverse and the gates on the third stream test done; the streamed
    A^T dy releases progress words (at_epoch advances on the host for dead launches too).  The factor after a stop is that of
    iterate K, so it is recorded after K = 0 as well."""
    env, want = OVERLAP[variant]
    A, b, c = _syn(2048, 2500, 7)
    _cell(monkeypatch, "overlap-16-blocks-" + variant, lambda ce: ipm.IpmSolver(A, b, c, check_every=ce), env=env, overlap=True,
          check=lambda sv: _words(sv, blocks=16, grouped_trsv=1, device_polling=1, fused_small=0, **want))


@pytest.mark.parametrize("variant", sorted(OVERLAP))
def test_overlap_factor_solves_after_a_stop(monkeypatch, variant):
    """What the overlap path promises after a stop -- B / invD hold the complete factor of the final iterate -- has a user:
    normal_solve(rhs, reuse_factor=True).  Its substitutions read the factor AND the explicit inverses of the diagonal groups, which
    enqueue_iteration forms on the third stream behind the factorization; formation and factorization of the firing iteration run
    whole (latch done_f), so the group inverses have to as well, or the solve pairs the factor of iterate K with inverses of iterate
    K - 1.  After solve(max_iter=3) under c = 1, 3, 5 (D = 0, 2, 1): z1 = normal_solve(rhs, reuse_factor=True) and L1 = get_factor();
    then on the same handle z2 = normal_solve(rhs, d = x / s), which forms, factors and inverts from the final iterate with nothing
    running ahead, and L2.  z1 and L1 equal those of c = 1 byte for byte.  Where L1 and L2 are the same bytes (the serial
    factorization: the same kernels on the same d), z1 and z2 must be too.  Where they are not (the fused launch sums the formation
    in another order), both are Cholesky solves of the same B = A diag(x / s) A^T, each with a normwise backward error of at most
    (3 m + 1) u for factorization and substitutions (Higham, Accuracy and Stability, thm 10.4) plus n u for the sums of the
    formation, so |z1 - z2| <= 2 kappa (3 m + n + 2) u |z2| with kappa = (|L2|_F |L2^-1|_F)^2 >= kappa_2(B).  Stale inverses miss
    that by many orders: d moves by whole factors between two early iterates."""
    from scipy.linalg import solve_triangular
    env, want = OVERLAP[variant]
    A, b, c = _syn(2048, 2500, 7)
    m, n = A.shape
    rhs = np.random.default_rng(21).standard_normal(m)
    with monkeypatch.context() as mp:
        for k in CLEARED:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        first = None
        for ce in (1, 3, 5):
            with ipm.IpmSolver(A, b, c, check_every=ce) as sv:
                sv.init_state(Y0)
                st = sv.solve(tol=1e-8, max_iter=3)
                assert st["status"] == 2 and st["iterations"] == 3, st
                _words(sv, blocks=16, grouped_trsv=1, device_polling=1, **want)
                L1 = sv.get_factor()
                z1 = sv.normal_solve(rhs, reuse_factor=True)
                x, _, s = sv.get_state()
                z2 = sv.normal_solve(rhs, d=x / s)
                L2 = sv.get_factor()
                assert sv.schedule()["timeouts_recovered"] == 0
            same = L1.tobytes() == L2.tobytes()
            if same:
                err, bound = float(np.max(np.abs(z1 - z2))), 0.0
            else:
                Li = solve_triangular(np.tril(L2), np.eye(m), lower=True)
                kappa = (np.linalg.norm(np.tril(L2)) * np.linalg.norm(Li)) ** 2
                err, bound = float(np.linalg.norm(z1 - z2) / np.linalg.norm(z2)), 2.0 * kappa * (3 * m + n + 2) * 2.0 ** -53
            print("RUN-AHEAD overlap-solve-%s: c = %d  K = 3  D = %d  factors bytewise equal %s  |z1 - z2| = %.3e  bound %.3e"
                  % (variant, ce, dead(ce, 3), same, err, bound))
            assert err <= bound, (variant, ce, err, bound)
            if first is None:
                first = L1.tobytes(), z1.tobytes()
            else:
                assert first[0] == L1.tobytes() and first[1] == z1.tobytes(), (variant, ce, "against c = 1")


@pytest.mark.parametrize("list_form", [1, 0])
def test_sparse_A_dense_factor(monkeypatch, list_form):
    """130 x 257 as CSC, bounded: B from the product list and, with IPM_LIST_FORM=0, from the row-owner kernel (no schedule word
    tells the two apart: the cells rest on the library's rule and on the switch, as in test_gpu_residue.py)."""
    A, b, c, ub = _sparse130()

    def check(sv):
        assert sv.sparse and sv.factor == "dense" and sv.bounded == int(np.isfinite(ub).sum())
        return _words(sv, blocks=2, fused_small=0, fused_factor=0)
    _cell(monkeypatch, "sparse-A-list-form-%d" % list_form, lambda ce: ipm.IpmSolver(A, b, c, ub=ub, factor="dense", check_every=ce),
          env={} if list_form else {"IPM_LIST_FORM": "0"}, check=check, ub=ub)


def test_tile_envelope(monkeypatch):
    """500 rows, reorder=None: tile (3, 0) lies outside the envelope and no kernel touches it."""
    A, b, c = _block_bidiagonal()

    def check(sv):
        assert sv.sparse and sv._perm is None
        return _words(sv, blocks=4, envelope=1, fused_small=0)
    _cell(monkeypatch, "tile-envelope", lambda ce: ipm.IpmSolver(A, b, c, factor="dense", reorder=None, check_every=ce), check=check)


SPARSE_FACTOR = [("path300", "task", {}), ("path300", "level", {}), ("bigborder_300_20", "task", {}), ("bigborder_300_20", "level", {}),
                 ("path300", "task", {"IPM_SP_FUSE_FWD": "0"})]


@pytest.mark.parametrize("name,mode,extra", SPARSE_FACTOR, ids=["%s-%s%s" % (n, m, "-unfused-fwd" if e else "") for n, m, e in SPARSE_FACTOR])
def test_sparse_factor(monkeypatch, name, mode, extra):
    """The tree sweeps: sp_epoch advances on the host for launches that return at entry on the device; the task walk polls hand-off
    flags, the level walk does not; IPM_SP_FUSE_FWD=0 takes the predictor's forward sweep off the factorization."""
    A, b, c, ub = _feasible(SC.iteration_case(name, False))
    A = sparse.csc_matrix(A)
    t = SC.tree(name)

    def check(sv):
        fi = sv.factor_info()
        assert sv.factor == "sparse" and (fi["panels"], fi["height"], fi["widest_front"]) == (t.nsn, t.height, t.rmax), fi
        return _words(sv, sparse_level_mode=1 if mode == "level" else 0, fused_small=0)
    _cell(monkeypatch, "sparse-factor-%s-%s%s" % (name, mode, "-unfused-fwd" if extra else ""),
          lambda ce: ipm.IpmSolver(A, b, c, ub=ub, factor="sparse", check_every=ce), env=dict(extra, IPM_SP_MODE=mode), check=check, ub=ub)


def test_centrality_correctors(monkeypatch):
    """130 x 257 dense with two corrector rounds: their products and substitutions test MccCtl::rdone, which the round's target kernel
    sets from done; the tallies (corrector_info) must not count a dead round."""
    A, b, c = _syn(130, 257, 11)

    def check(sv):
        assert sv.correctors == 2
        return _words(sv, blocks=2, fused_small=0, fused_factor=0)
    _cell(monkeypatch, "correctors-2", lambda ce: ipm.IpmSolver(A, b, c, correctors=2, check_every=ce), check=check)


def test_small_path_ignores_check_every(monkeypatch):
    """AFIRO: the loop is one launch of one workgroup; check_every has no effect there (c = 1 and c = 7 only, no dead tail to cover)."""
    A, b, c = IC.netlib("AFIRO")
    runs = tuple((ce, K) for K in (0, 2, 3) for ce in (1, 7))
    _cell(monkeypatch, "small-AFIRO", lambda ce: ipm.IpmSolver(A, b, c, check_every=ce), runs=runs, tails=False,
          check=lambda sv: _words(sv, blocks=1, fused_small=1))


# ---- stops by the other branches of the stop test --------------------------------------------------------------------------
def _free_runs(cs=CS):
    return tuple((c, 200) for c in cs)


def _converged_tails(got):
    """The realised D include 0 and at least two different nonzero values."""
    ds = {dead(c, K) for c, K in got}
    assert 0 in ds and len(ds - {0}) >= 2, sorted(ds)


CONVERGE = {"dense-2-blocks": (lambda: _syn(130, 257, 11) + (None,), {}, dict(blocks=2, fused_factor=0), False, 1e-8),
            "sparse-A": (_sparse130, dict(factor="dense"), dict(blocks=2, fused_small=0), False, 1e-8),
            "dense-9-blocks": (lambda: _syn(1100, 1400, 12) + (None,), {}, dict(blocks=9, device_polling=1), False, 1e-7),
            "overlap-16-blocks": (lambda: _syn(2048, 2500, 7) + (None,), {}, dict(blocks=16, fused_factor=1, stream_at=1), True, 1e-7)}


@pytest.mark.parametrize("cell", sorted(CONVERGE))
def test_convergence(monkeypatch, cell):
    """Status 1, K as it comes.  tol = 1e-8, except for the 9-block and the 16-block LP: both converge there after K = 19 iterations,
    and K + 1 = 20 divides by 2, 4 and 5 (D = 0, 0, 1, 0, 0, 1: one nonzero value only), so they run at tol = 1e-7."""
    lp, kw, want, overlap, tol = CONVERGE[cell]
    A, b, c, ub = lp()
    got = _cell(monkeypatch, "converge-" + cell, lambda ce: ipm.IpmSolver(A, b, c, ub=ub, check_every=ce, **kw), runs=_free_runs(), max_iter=200,
                status=1, tol=tol, overlap=overlap, ub=ub, tails=False, check=lambda sv: _words(sv, **want))
    _converged_tails(got)


@pytest.mark.parametrize("name", ["primal_dense", "dual_dense"])
def test_detection(monkeypatch, name):
    """Status 5 / 6 (detect_fire in the stop test): 40 x 90 dense, one block on the multi-kernel path; the certificate is recorded."""
    P = IC.small_instances()[name]()
    got = _cell(monkeypatch, "detect-" + name, lambda ce: ipm.IpmSolver(P["A"], P["b"], P["c"], detect_infeasibility=True, check_every=ce),
                env={"IPM_FUSED_SMALL": "0"}, runs=_free_runs(), max_iter=200, status=IC.KIND[P["kind"]], tails=False,
                check=lambda sv: _words(sv, blocks=1, fused_small=0))
    assert 0 in {dead(c, K) for c, K in got}


def test_nan(monkeypatch):
    """Status 3: x1 + x2 = -1, x >= 0 (the LP of test_nan_solve_returns_last_finite_objective) drives the iterate to NaN;
    objective_last_finite is part of the statistics.  IPM_FUSED_SMALL=0 puts the 1 x 2 LP on the multi-kernel path."""
    A, b, c = sparse.csc_matrix(np.array([[1.0, 1.0]])), np.array([-1.0]), np.array([1.0, 2.0])
    got = _cell(monkeypatch, "nan", lambda ce: ipm.IpmSolver(A, b, c, check_every=ce), env={"IPM_FUSED_SMALL": "0"}, runs=_free_runs(),
                max_iter=999, status=3, tails=False, check=lambda sv: _words(sv, blocks=1, fused_small=0))
    assert 0 in {dead(c, K) for c, K in got}


def test_automatic_shift(monkeypatch):
    """200 rows, one guarded pivot more than 5 %: ipm_solve restarts from its snapshot with the Tikhonov shift after the FIRST CHUNK,
    whatever its length -- with c >= 4 that chunk already holds the stop at K = 3 and dead launches behind it, all rolled back.  No
    iterate(K) oracle: ipm_iterate never takes the shift."""
    case = PG._five_pct_case(200, auto_shift_boundary(200) + 1)
    A, b, c = PG._lp(case)

    def start(sv):
        x, s = case.x_state()
        sv.set_state(x, np.zeros(case.m), s)

    def check(sv):
        assert sv.stats["auto_regularized"] == 1, sv.stats
        return _words(sv, blocks=2, fused_small=0)
    _cell(monkeypatch, "auto-shift", lambda ce: ipm.IpmSolver(A, b, c, factor="dense", reorder=None, check_every=ce),
          runs=tuple((ce, 3) for ce in CS), oracle=False, start=start, check=check, tails=False)


# ---- the lockstep batch ----------------------------------------------------------------------------------------------------
LS_CAPS = (1, 3, 6)


def _ls_problems():
    A, b, c, _ = _feasible(IO.get("lock/" + IO.shape_name(*IO.SMALL, False)))
    return [(sparse.csc_matrix(A), b, c), _sparsified(300, 600, 13, 0.05), _sparsified(520, 700, 15, 0.04)]


def _ls_obs(sv):
    o = Obs()
    o.put("stats", sv.stats)
    o.put("state", sv.get_state())
    o.put("history", sv.history())
    assert sv.schedule()["timeouts_recovered"] == 0
    return o


def _ls_batch(probs, ces, late):
    """The three LPs with check_every `ces` in one batch, per-handle caps LS_CAPS through ipm_batch_add; late: the first handle joins
    after the first step -> (records per LP, the LPs each step reported)."""
    lib = _lib.load()
    svs = [ipm.IpmSolver(*p, lockstep=True, factor="dense", check_every=ce) for p, ce in zip(probs, ces)]
    bt = C.c_void_p()
    try:
        for sv, blocks in zip(svs, (2, 3, 5)):
            assert ipm.lockstep_eligible(sv) and sv.schedule()["blocks"] == blocks
            sv.init_state(Y0)
        assert lib.ipm_batch_create(0, None, C.byref(bt)) == _lib.IPM_OK
        members, steps = [], []

        def add(i):
            idx = C.c_int32(-1)
            rc = lib.ipm_batch_add(bt, svs[i]._h, 1e-8, 1e-8, 1e-8, LS_CAPS[i], C.byref(idx))
            assert rc == _lib.IPM_OK and idx.value == len(members), (rc, lib.ipm_batch_last_error(bt))
            members.append(i)

        def step():
            fin, nf, na = (C.c_int32 * 3)(), C.c_int32(0), C.c_int32(0)
            assert lib.ipm_batch_step(bt, fin, 3, C.byref(nf), C.byref(na)) == _lib.IPM_OK, lib.ipm_batch_last_error(bt)
            out = []
            for k in range(nf.value):
                st = _lib.Stats()
                assert lib.ipm_batch_stats(bt, fin[k], C.byref(st)) == _lib.IPM_OK
                svs[members[fin[k]]].stats = st.as_dict()
                out.append(members[fin[k]])
            steps.append(sorted(out))
            return na.value
        for i in ((1, 2) if late else (0, 1, 2)):
            add(i)
        active = step()
        if late:
            add(0)
        for _ in range(4):
            if not active and len(members) == 3:
                break
            active = step()
        assert active == 0
        return [_ls_obs(sv) for sv in svs], steps
    finally:
        if bt:
            lib.ipm_batch_destroy(bt)
        for sv in svs:
            sv.close()


def test_lockstep_batch(monkeypatch):
    """Three sparse LPs on the dense-tile factor (2, 3 and 5 blocks) with check_every 1, 3, 5 and caps 1, 3, 6: the batch runs chunks
    of max(check_every) = 5, so the first LP is dead for 3 iterations of the first chunk while its neighbours are live, the second for
    1, and the third stops in the second chunk (D = 3).  Each LP's record equals the same LP solved alone by ipm_solve at
    check_every = 1.  Again with the check_every values permuted, and with the first LP joining after the first step."""
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)
    probs = _ls_problems()
    alone = []
    for p, cap in zip(probs, LS_CAPS):
        with ipm.IpmSolver(*p, lockstep=True, factor="dense", check_every=1) as sv:
            sv.init_state(Y0)
            st = sv.solve(tol=1e-8, max_iter=cap)
            assert st["status"] == 2 and st["iterations"] == cap, st
            alone.append(_ls_obs(sv))
    for ces, late, want_steps in (((1, 3, 5), False, [[0, 1], [2]]), ((5, 1, 3), False, [[0, 1], [2]]), ((3, 5, 1), False, [[0, 1], [2]]),
                                  ((1, 3, 5), True, [[1], [0, 2]])):
        got, steps = _ls_batch(probs, ces, late)
        print("RUN-AHEAD lockstep: check_every %s, chunk 5, late join %s: finished per step %s; D = %s"
              % (ces, late, steps, [dead(5, K) for K in LS_CAPS]))
        assert steps == want_steps, steps
        for i, (a, g) in enumerate(zip(alone, got)):
            differ = _first_difference(a, g)
            assert not differ, ("lockstep LP %d, check_every %s, late %s, against ipm_solve alone" % (i, ces, late), differ)
