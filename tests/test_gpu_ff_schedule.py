"""GPU tests (-m gpu) of the fused formation + factorization (csrc/form_factor.h, form_factor_roles_kernel) across its work list
(csrc/ff_schedule.h).  The list is a pure function of (nblk, Q, workers, model) and only the ORDER of its items depends on the
duration model; every tile's arithmetic order is fixed by the K-chunk cuts, the column batches, the seq chain and the single
ADD_BASE item.  So:
  a. any valid reordering (IPM_FF_MODEL perturbations, proven by tests/test_ff_schedule.py to reorder without changing an item)
     and the instrumented kernel instantiation (IPM_FF_PROF, IPM_FF_TRACE_ITEMS) give a BIT-IDENTICAL factor and iterate -- a
     missing or too-weak acquire in a hand-off would show up as a different result under a different order;
  b. every chunking knob (which does change the arithmetic) stays within LAPACK bounds, including empty formation chunks;
  c. the round-3 structure (IPM_FF_CHAIN_MODE=0) is refused at handle creation (it met a recovered hand-off time-out);
  d. the block counts up to FF_MAX_NBLK = 96 that only the largest work lists reach (unsigned char item fields, slab sizes).
A fresh IpmSolver per setting: the knobs are read when the handle builds its list.  Every fused run asserts fused_factor == 1 and
no recovered hand-off time-out.  Measured values are printed with a "[ff]" prefix (pytest -s)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                              # noqa: E402
from ff_cases import KNOBS, MODELS, pair_chunks                     # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp         # noqa: E402

SCALARS = ("status", "iterations", "pivots_fixed", "objective", "rp_norm", "rd_norm", "gap", "mu", "mu_aff", "sigma",
           "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d")


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


def _run(monkeypatch, A, b, c, env, steps, state=None, fused=True):
    """One fresh handle under `env`: `steps` iterations from init_state(0.0) or from `state` = (x, y, s)."""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        with ipm.IpmSolver(A, b, c) as sv:
            if state is None:
                sv.init_state(0.0)
            else:
                sv.set_state(*state)
            st = sv.iterate(steps)
            x, y, s = sv.get_state()
            L = sv.get_factor()
            sch = sv.schedule()
    if fused is not None:
        assert sch["fused_factor"] == int(fused), f"{env} {sch}"
    assert sch["timeouts_recovered"] == 0, f"{env} {sch}"
    return {"st": {k: st[k] for k in SCALARS}, "x": x, "y": y, "s": s, "L": L}


def _bitwise(r0, r1, what):
    for k in ("L", "x", "y", "s"):
        assert np.array_equal(r0[k], r1[k]), (what, k, rel(r1[k], r0[k]))
    assert r0["st"] == r1["st"], (what, r0["st"], r1["st"])


# ---------------------------------------------------------------------------------------------- a. bitwise order invariance
@pytest.mark.parametrize("m", [2048, 4096, 4200])          # 16, 32 and 33 blocks (ragged last block); n = 8192: 512 stages, i.e.
def test_reordered_work_lists_give_bit_identical_results(monkeypatch, m):   # the host list of tests/test_ff_schedule.py
    A, b, c = synthetic_lp(m, 8192, seed=7)
    base = {"IPM_FUSED_FACTOR": "1"}
    r0 = _run(monkeypatch, A, b, c, base, 2)
    for model in MODELS:
        _bitwise(r0, _run(monkeypatch, A, b, c, {**base, "IPM_FF_MODEL": model}, 2), model)
    for instr in ("IPM_FF_PROF", "IPM_FF_TRACE_ITEMS"):     # form_factor_roles_kernel<true>: instrumentation changes no bit
        _bitwise(r0, _run(monkeypatch, A, b, c, {**base, instr: "1"}, 2), instr)


# ------------------------------------------------------------------------------- b. chunking knobs against a host reference
M_B, N_B = 2048, 4100                                       # 16 blocks, np = 4160: not a multiple of 8192


@pytest.fixture(scope="module")
def lp_b():
    return synthetic_lp(M_B, N_B, seed=2)


def _state(kind, n, m):
    rng = np.random.default_rng(9)
    y = rng.standard_normal(m)
    if kind == "benign":                                    # d = x / s in [0.25, 4]
        return rng.uniform(0.5, 2.0, n), y, rng.uniform(0.5, 2.0, n)
    e = rng.uniform(-4.0, 4.0, n)                           # a late iterate: d spans 1e-8 ... 1e8
    e[:2] = (-4.0, 4.0)
    return 10.0 ** e, y, 10.0 ** -e


@pytest.fixture(scope="module")
def refs_b(lp_b):
    A = lp_b[0]
    out = {}
    for kind in ("benign", "wide"):
        x, y, s = _state(kind, N_B, M_B)
        B = (A * (x / s)) @ A.T
        out[kind] = ((x, y, s), B, np.linalg.cholesky(B))
    return out


# rel(L, L_lapack) on the wide state: B's conditioning makes the two factors differ far more than on the benign state, for any
# correct factorization.  Measured on the MI355X: 1.7e-11 with the default knobs, 1.0e-11 ... 6.9e-11 over the knobs below
# (IPM_FF_Q=1 the largest); the bound sits just above the worst knob.  The scaled backward error stays at 0.8e-15 ... 2.3e-15.
WIDE_REL = 1e-10


def _check_factor(L, B, Lref, kind, what):
    be = float(np.linalg.norm(L @ L.T - B) / np.linalg.norm(B))
    r = rel(L, Lref)
    print(f"[ff] {what} {kind}: backward {be:.3e}, rel to LAPACK {r:.3e}")
    assert be <= 1e-13, (what, kind, be)
    assert r <= (1e-10 if kind == "benign" else WIDE_REL), (what, kind, r)


@pytest.mark.parametrize("var,val", [(None, None), ("IPM_FF_Q", "1"), ("IPM_FF_Q", "2"), ("IPM_FF_Q", "3"), ("IPM_FF_Q", "7"),
                                     ("IPM_FF_Q", "16")] + KNOBS)
@pytest.mark.parametrize("kind", ["benign", "wide"])
def test_chunking_knob_factor_against_lapack(monkeypatch, lp_b, refs_b, kind, var, val):
    """One iteration from a set state: the factor is the Cholesky factor of B = A diag(x/s) A^T, with each knob alone."""
    A, b, c = lp_b
    state, B, Lref = refs_b[kind]
    env = {"IPM_FUSED_FACTOR": "1"}
    if var:
        env[var] = val
    r = _run(monkeypatch, A, b, c, env, 1, state=state)
    _check_factor(r["L"], B, Lref, kind, f"{var}={val}")


def test_empty_formation_chunks(monkeypatch):
    """4 blocks, n = 448: 28 formation stages cut into 16 chunks per pair with lengths spread by 0.9 -- some chunks have no
    stage at all (the kernel's `s1 > s0` branch: the slab is written as zeros).  The host restatement of the cut formula shows
    they exist; the factor still matches LAPACK."""
    m, n = 400, 448
    cuts = pair_chunks(4, 16, n // 16, stagger=0.9)
    empty = sum(1 for v in cuts.values() for s0, s1 in v if s0 == s1)
    assert empty >= 1
    A, b, c = synthetic_lp(m, n, seed=4)
    rng = np.random.default_rng(1)
    x, s, y = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n), rng.standard_normal(m)
    r = _run(monkeypatch, A, b, c, {"IPM_FUSED_FACTOR": "force", "IPM_FF_Q": "16", "IPM_FF_STAGGER": "0.9"}, 1, state=(x, y, s))
    B = (A * (x / s)) @ A.T
    _check_factor(r["L"], B, np.linalg.cholesky(B), "benign", f"empty chunks ({empty})")


# ------------------------------------------------------------------------------------------------------------- c. chain mode 0
def test_chain_mode_0_is_refused(monkeypatch):
    """IPM_FF_CHAIN_MODE=0 (the round-3 structure: the chain as three launches per step beside 224 workers) met a recovered
    hand-off time-out at 16 blocks, so the library refuses it when the handle is created instead of leaving a fused
    launch selectable that can spin to its time-out bound.  The default mode stays fused on the same LP right after."""
    A, b, c = synthetic_lp(2048, 4100, seed=5)
    with monkeypatch.context() as mp:
        mp.setenv("IPM_FUSED_FACTOR", "1")
        mp.setenv("IPM_FF_CHAIN_MODE", "0")
        with pytest.raises(ipm.IpmError, match="IPM_FF_CHAIN_MODE=0"):
            ipm.IpmSolver(A, b, c)
    r = _run(monkeypatch, A, b, c, {"IPM_FUSED_FACTOR": "1", "IPM_FF_CHAIN_MODE": "1"}, 3)
    r0 = _run(monkeypatch, A, b, c, {"IPM_FUSED_FACTOR": "0"}, 3, fused=False)
    assert rel(r["L"], r0["L"]) < 1e-10


# ---------------------------------------------------------------------------------------------- d. block counts up to the limit
def _probe_backward(L, A, d, rng, k=8):
    """max over k random v of ||L (L^T v) - A (d o (A^T v))|| / (||A||_2^2 ||d||_inf ||v||): O(mn) per probe, no m^3 host work.
    ||A||_2 from power iterations (a lower estimate, so the ratio is if anything overstated)."""
    u = rng.standard_normal(A.shape[1])
    for _ in range(8):
        u = A.T @ (A @ u)
        u /= np.linalg.norm(u)
    a2 = float(np.linalg.norm(A.T @ (A @ u)))                # ~ ||A||_2^2
    worst = 0.0
    for _ in range(k):
        v = rng.standard_normal(A.shape[0])
        r = L @ (L.T @ v) - A @ (d * (A.T @ v))
        worst = max(worst, float(np.linalg.norm(r) / (a2 * float(np.max(d)) * np.linalg.norm(v))))
    return worst


@pytest.mark.parametrize("m,max_nblk,want", [
    (9216, None, 1),                 # 72 blocks: the default rule's upper end
    (9100, None, 1),                 # 72 blocks, ragged
    (9300, None, 0),                 # 73 blocks: declined by default
    (9300, "96", 1),                 # IPM_FF_MAX_NBLK lifts the rule ...
    (12288, "96", 1),                # ... up to FF_MAX_NBLK
    (12300, "200", 0),               # 97 blocks: never (the unsigned char fields and the slab layout stop at 96)
])
def test_block_counts_up_to_the_limit(monkeypatch, m, max_nblk, want):
    n = 2 * m
    rng = np.random.default_rng(m)
    A = rng.standard_normal((m, n))
    b, c = A @ np.ones(n), A.T @ np.ones(m) + 1.0
    x, s, y = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n), rng.standard_normal(m)
    env = {"IPM_FF_MAX_NBLK": max_nblk} if max_nblk else {}
    r1 = _run(monkeypatch, A, b, c, env, 1, state=(x, y, s), fused=bool(want))
    if not want:
        return
    L1 = r1.pop("L")
    del r1
    r0 = _run(monkeypatch, A, b, c, {"IPM_FUSED_FACTOR": "0"}, 1, state=(x, y, s), fused=False)
    rl = rel(L1, r0["L"])
    del r0
    be = _probe_backward(L1, A, x / s, rng)
    print(f"[ff] {m} rows ({(m + 127) // 128} blocks): rel L to serial {rl:.3e}, probe backward {be:.3e}")
    assert rl < 1e-10
    assert be <= 1e-13
