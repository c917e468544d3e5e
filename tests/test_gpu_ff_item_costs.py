"""GPU tests (-m gpu) of the update items' base add in the fused launch (csrc/form_factor.h, the HEAD instantiation of
form_factor_body).  STREAMED base add: new tile = old tile + slab 0 + ... + slab qn - 1 runs as rounds (slab, register group)
with a fixed number in flight in a ring of register slots, from the loads of the old tile to the last round of the last slab,
refilled across the slab boundaries; every element still receives its addends in the same order.  No rounded operation
changes, so the launch must stay BIT-IDENTICAL to form_factor_roles_kernel (IPM_FF_REF_ENGINE=1), which keeps the
slab-at-a-time add.  Shapes: the smallest at which the new code can go wrong --
  * 16 blocks (2048 x 4096, the smallest fused size): tiles (0,0) and (1,0) have a single item, INIT with ADD_BASE -- the
    stream starts at slab 0 with no old tile in front;
  * 21 blocks (2600 x 5300): the odd block count makes the last pair half-live, and the ragged last block puts the padding
    unit diagonal behind the base add;
each with IPM_FF_Q unset, 1 and 3, so that 4, 1 and 3 slabs per tile go through the ring (1: the peeled last slab alone; 3 and
4: the loop refills across two and three slab boundaries).  Factor, iterate and the iteration scalars after 3 iterations.
(The one-poll wait for an item's inputs that was built with it was taken out again -- DESIGN.md 4-F -- so the waits are the
parent's; their give-up path is driven by tests/test_gpu_recovery.py.  The recorded digests are compared by
tests/test_gpu_ff_engines.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                              # noqa: E402
import test_gpu_ff_engines as eng                                  # noqa: E402

SCALARS = ("status", "iterations", "pivots_fixed", "objective", "rp_norm", "rd_norm", "gap", "mu", "mu_aff", "sigma",
           "alpha_aff_p", "alpha_aff_d", "alpha_p", "alpha_d")
SIZES = {16: (2048, 4096), 21: (2600, 5300)}                       # blocks -> (m, n)


def _run(monkeypatch, lp, env, steps=3):
    A, b, c, state = lp
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        with ipm.IpmSolver(A, b, c) as sv:
            sv.set_state(*state)
            st = sv.iterate(steps)
            x, y, s = sv.get_state()
            L = sv.get_factor()
            sch = sv.schedule()
    assert sch["fused_factor"] == 1 and sch["timeouts_recovered"] == 0, (env, sch)
    return {"st": {k: st[k] for k in SCALARS}, "x": x, "y": y, "s": s, "L": L}, sch


@pytest.fixture(scope="module", params=sorted(SIZES))
def lp(request):
    return (request.param,) + eng.problem(*SIZES[request.param])


@pytest.mark.parametrize("q", [None, "1", "3"])
def test_streamed_base_add_bitwise_equal_to_reference_launch(monkeypatch, lp, q):
    nblk, prob = lp[0], lp[1:]
    env = {"IPM_FUSED_FACTOR": "force"}
    if q is not None:
        env["IPM_FF_Q"] = q
    r, sch = _run(monkeypatch, prob, env)
    assert sch["blocks"] == nblk, sch
    ref, _ = _run(monkeypatch, prob, {**env, "IPM_FF_REF_ENGINE": "1"})
    for k in ("L", "x", "y", "s"):
        assert np.array_equal(r[k], ref[k]), (nblk, q, k)
    assert r["st"] == ref["st"], (nblk, q, r["st"], ref["st"])
    assert np.all(np.isfinite(r["L"])) and np.all(np.diag(r["L"]) > 0)
    assert not np.any(np.triu(r["L"], 1))
