"""GPU tests (-m gpu) of the explicit group inverses of the grouped triangular solves (csrc/ginv_gemm_f64.h, enqueue_group_inverses
in csrc/host_factor_solve.h).  Per level of the recursive doubling the default path runs one launch for S = XT11 L21^T and one that
produces X21 = -X22 S^T and XT12 = -S X22^T together, on an engine of their own that keeps several stages of global loads in
flight.  Per accumulator the MFMA sequence, its operands and their roles are those of the three launches of the generic kernel that
IPM_GINV_REF=1 selects, so no bit may differ:

  whole inverses   solve_linear on B = M M^T + I (the construction of tests/test_gpu_chol_factor_bits.py); every X_g and XT_g,
                   zero triangles included, against the reference path, and max |X_g L_gg - I| <= 1e-10 with L from get_factor, so
                   that two equal wrong answers do not pass.  Sizes: groups of 2, 4 and 8 blocks (levels up to hs = 128, 256, 512),
                   1, 2 and 3 groups, padding rows (m = 1000), a ragged block count (18 blocks: two groups and two blocks over);
  partial ranges   a dense LP of 16 blocks with and without the fused formation + factorization: groups [0, nG - 1) go to the
                   residual stream behind the first gate (or from inside the serial factorization), the last group follows the
                   factorization; (x, y, s) and the scalars after iterate(2) against the reference path."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                              # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp         # noqa: E402

# m -> what schedule() must report: (blocks, blocks per group); groups = blocks // blocks per group
WHOLE = {256: (2, 2), 512: (4, 4), 1000: (8, 8), 2304: (18, 8), 3072: (24, 8)}


def with_env(env, fn):
    """fn() with exactly these switches set (a handle reads them when it is created), the environment restored afterwards."""
    keys = set(env) | {"IPM_GINV_REF"}
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def spd(m):
    rng = np.random.default_rng(4000 + m)
    M = rng.standard_normal((m, 64))
    B = M @ M.T + np.eye(m)
    rhs = rng.standard_normal(m)
    for a in (B, rhs):
        a.setflags(write=False)
    return B, rhs


def inverses(m):
    B, rhs = spd(m)
    with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
        z, nfix = sv.solve_linear(B, rhs)
        sch = sv.schedule()
        assert nfix == 0 and sch["grouped_trsv"] == 1 and sch["timeouts_recovered"] == 0, sch
        groups = sch["blocks"] // sch["group_blocks"]
        X = [sv.debug_group_inverse(g, 0) for g in range(groups)]
        XT = [sv.debug_group_inverse(g, 1) for g in range(groups)]
        return X, XT, sv.get_factor(), z, sch


@pytest.mark.parametrize("m", sorted(WHOLE))
def test_group_inverses_bitwise_equal_to_three_launch_reference(m):
    blocks, gsz = WHOLE[m]
    X, XT, L, z, sch = with_env({}, lambda: inverses(m))
    Xr, XTr, Lr, zr, schr = with_env({"IPM_GINV_REF": "1"}, lambda: inverses(m))
    assert (sch["blocks"], sch["group_blocks"]) == (blocks, gsz) and schr == sch, (sch, schr)
    assert len(X) == blocks // gsz and len(Xr) == len(X)
    assert np.array_equal(L, Lr) and np.array_equal(z, zr)
    rows = 128 * gsz
    Lp = np.eye(128 * blocks)                                       # padding rows of the factor: the identity
    Lp[:m, :m] = L
    for g in range(len(X)):
        assert X[g].shape == (rows, rows)
        assert X[g].tobytes() == Xr[g].tobytes(), ("X", g)          # (bytes: signed zeros and the zero triangle count)
        assert XT[g].tobytes() == XTr[g].tobytes(), ("XT", g)
        assert np.array_equal(XT[g], X[g].T), g
        assert not np.any(np.triu(X[g], 1)), g
        Lgg = Lp[g * rows:(g + 1) * rows, g * rows:(g + 1) * rows]
        err = float(np.max(np.abs(X[g] @ Lgg - np.eye(rows))))
        print("FIGURE m=%d group %d of %d: max |X L - I| = %.3e (bound 1e-10)" % (m, g, len(X), err))
        assert err <= 1e-10


@functools.lru_cache(maxsize=None)
def lp16():
    A, b, c = synthetic_lp(2048, 2500, seed=7)
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c


def two_iterations():
    A, b, c = lp16()
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        st = sv.iterate(2)
        return sv.get_state(), st, sv.schedule()


@pytest.mark.parametrize("fused", ["0", "force"])
def test_partial_ranges_on_the_residual_stream_bitwise_equal_to_reference(fused):
    (x, y, s), st, sch = with_env({"IPM_FUSED_FACTOR": fused}, two_iterations)
    (xr, yr, sr), str_, schr = with_env({"IPM_FUSED_FACTOR": fused, "IPM_GINV_REF": "1"}, two_iterations)
    assert sch == schr and sch["blocks"] == 16 and sch["group_blocks"] == 8 and sch["timeouts_recovered"] == 0, (sch, schr)
    assert sch["fused_factor"] == (1 if fused == "force" else 0), sch
    assert st["iterations"] == 2 and np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(s))
    for name, a, r in (("x", x, xr), ("y", y, yr), ("s", s, sr)):
        assert a.tobytes() == r.tobytes(), name
    assert set(st) == set(str_)
    for k in sorted(set(st) - {"solve_ms"}):                        # (solve_ms is wall time)
        assert np.array_equal(np.asarray(st[k]), np.asarray(str_[k])), (k, st[k], str_[k])
