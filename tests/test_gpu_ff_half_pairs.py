"""GPU tests (-m gpu) of the half-live formation engine (csrc/form_factor.h, ff_gemm_pair<HEAD, HALF>): a tile pair whose
upper tile lies above the diagonal (c = 2r + 1) or whose lower tile lies below the matrix (odd block count, last row pair)
is formed by the four waves of the live tile alone; the dead half is neither loaded, staged nor multiplied.  Every live wave
runs the MFMA sequence of the full pair, so the launch must stay BIT-IDENTICAL to form_factor_roles_kernel
(IPM_FF_REF_ENGINE=1), which keeps computing both halves on a stand-in panel:
  * 16 blocks (the smallest fused size: every odd block column has an upper-dead pair) and 21 blocks with a ragged last block
    (m = 2600: the last row pair is lower-dead, pair (20, 20) is a single tile), each under the default chunking and under
    IPM_FF_Q = 1 and 3: factor, iterate and the iteration scalars after 3 iterations, bit for bit;
  * dead storage: the debug entry points cannot pre-fill B or the slabs, and ipm_get_factor returns the lower triangle only, so
    the check that is available is the one above -- the lower factor is identical -- together with the code: a dead half's slab
    store sits behind the same `half == 0 ? up : lo` test as before, its slabs do not exist (tile_q counts live tiles only), and
    strictly upper tiles of B are written by no item.  The reference engine did not write them either;
  * the digests of tests/golden/ff_engine_factor.json (recorded with the previous stage schedule, read by
    tests/test_gpu_ff_engines.py) still match for the cases with dead halves.
max diag(B), the pivot guard's scale, comes from the FF_D items (not from this engine) and has no read-back entry point; it
enters every pivot test and, through pivots_fixed and the iterate, the scalars compared here."""
import json

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
def test_half_live_pairs_bitwise_equal_to_reference_launch(monkeypatch, lp, q):
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


@pytest.mark.parametrize("case", ["2048x4096", "2048x4096_q1", "2600x5300"])
def test_recorded_digests_still_match(case):
    m, n, env = eng.CASES[case]
    with open(eng.GOLDEN) as fh:
        want = json.load(fh)[case]
    A, b, c, state = eng.problem(m, n)
    r, sch = eng.run(A, b, c, state, env)
    assert sch["fused_factor"] == 1 and sch["timeouts_recovered"] == 0, sch
    assert eng.digests(r) == want
