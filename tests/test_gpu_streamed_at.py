"""GPU tests (-m gpu) of the streamed A^T dy (csrc/host_iteration.h: enqueue_normal_solve): the pass over A behind the
predictor's and the corrector's backward sweep is cut into row-chunk pieces that run on the residual stream as the sweep makes
their rows of dy final, released through a progress word that the sweep's own kernels store.  It is an overlap of work that stays
the same, so the checker is the handle with the switch off (IPM_STREAM_AT=0: one pass behind the sweep) and the bound is EQUALITY,
bit for bit.  Shapes: the smallest that reach each edge of the piece schedule (tests/test_at_pieces_host.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                              # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp         # noqa: E402

STAT_KEYS = ("status", "iterations", "objective", "rp_norm", "rd_norm", "gap", "mu", "mu_aff", "sigma", "alpha_aff_p", "alpha_aff_d",
             "alpha_p", "alpha_d", "pivots_fixed")


def _iterate(A, b, c, steps):
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        st = sv.iterate(steps)
        x, y, s = sv.get_state()
        return st, x, y, s, sv.schedule()


def _same_stats(st1, st0):
    keys = [k for k in STAT_KEYS if k in st0]
    assert len(keys) >= 10, sorted(st0)                              # (the names above are the statistics of the iterate)
    for k in keys:
        assert st1[k] == st0[k], (k, st1[k], st0[k])


# 2048 x 2500: two groups, 64-row chunks aligned to them -- 3072 x 3400: three groups, 96-row chunks that straddle both group
# boundaries -- 2300 x 2800: 18 blocks, two groups + two block steps (the diagonal gemv_n signals the first event)
@pytest.mark.parametrize("fused", ["0", "fused"])
@pytest.mark.parametrize("m,n,blocks", [(2048, 2500, 16), (3072, 3400, 24), (2300, 2800, 18)])
def test_three_iterations_are_bit_identical_to_the_single_pass(monkeypatch, m, n, blocks, fused):
    A, b, c = synthetic_lp(m, n, seed=7)
    if fused == "0":
        monkeypatch.setenv("IPM_FUSED_FACTOR", "0")
    monkeypatch.setenv("IPM_STREAM_AT", "0")
    st0, x0, y0, s0, sch0 = _iterate(A, b, c, 3)
    if fused != "0" and sch0["fused_factor"] != 1:                   # (where the default rule would not choose the fused launch)
        monkeypatch.setenv("IPM_FUSED_FACTOR", "force")
        st0, x0, y0, s0, sch0 = _iterate(A, b, c, 3)
    monkeypatch.delenv("IPM_STREAM_AT")
    st1, x1, y1, s1, sch1 = _iterate(A, b, c, 3)
    assert sch0["blocks"] == blocks and sch1["blocks"] == blocks and sch1["grouped_trsv"] == 1
    assert sch0["stream_at"] == 0 and sch1["stream_at"] == 1, (sch0, sch1)
    assert sch0["fused_factor"] == sch1["fused_factor"] == (0 if fused == "0" else 1)
    assert sch0["timeouts_recovered"] == 0 and sch1["timeouts_recovered"] == 0
    assert st1["iterations"] == 3
    assert np.array_equal(x1, x0) and np.array_equal(y1, y0) and np.array_equal(s1, s0)
    _same_stats(st1, st0)


def test_full_solve_matches_and_repeats_on_the_same_handle(monkeypatch):
    """2048 x 2500 to convergence: same iteration count and bit-identical final iterate as with the switch off; a second solve on the
    same handle (the progress word goes on counting: it is never cleared) repeats it bitwise; no time-out; the switch is reported."""
    A, b, c = synthetic_lp(2048, 2500, seed=9)
    monkeypatch.setenv("IPM_STREAM_AT", "0")
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        st0 = sv.solve(tol=1e-8, max_iter=200)
        x0, y0, s0 = sv.get_state()
        sch0 = sv.schedule()
    monkeypatch.delenv("IPM_STREAM_AT")
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        st1 = sv.solve(tol=1e-8, max_iter=200)
        x1, y1, s1 = sv.get_state()
        sch1 = sv.schedule()
        sv.init_state(0.0)
        st2 = sv.solve(tol=1e-8, max_iter=200)
        x2, y2, s2 = sv.get_state()
        sch2 = sv.schedule()
    assert sch0["stream_at"] == 0 and sch1["stream_at"] == 1 and sch2["stream_at"] == 1
    assert sch0["timeouts_recovered"] == 0 and sch1["timeouts_recovered"] == 0 and sch2["timeouts_recovered"] == 0
    assert st0["status"] == 1 and st1["status"] == 1 and st1["iterations"] == st0["iterations"]
    assert np.array_equal(x1, x0) and np.array_equal(y1, y0) and np.array_equal(s1, s0)
    _same_stats(st1, st0)
    assert st2["iterations"] == st1["iterations"]
    assert np.array_equal(x2, x1) and np.array_equal(y2, y1) and np.array_equal(s2, s1)
    _same_stats(st2, st1)


def test_a_handle_without_a_residual_stream_keeps_the_single_pass():
    """Below 16 blocks there is no residual stream: streaming is reported off, and the solve is what it was."""
    A, b, c = synthetic_lp(1500, 3100, seed=4)
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        st = sv.solve(tol=1e-8, max_iter=200)
        x, y, s = sv.get_state()
        sch = sv.schedule()
    assert sch["blocks"] == 12 and sch["stream_at"] == 0 and sch["timeouts_recovered"] == 0
    assert st["status"] == 1
    assert np.linalg.norm(A @ x - b) / (1 + np.linalg.norm(b)) < 1e-8
    assert np.linalg.norm(A.T @ y + s - c) / (1 + np.linalg.norm(c)) < 1e-8
    assert np.all(x > 0) and np.all(s > 0)
