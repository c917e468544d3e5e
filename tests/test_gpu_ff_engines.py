"""GPU tests (-m gpu) of the two GEMM engines inside the fused formation + factorization (csrc/form_factor.h): ff_gemm_pair
(formation chunks) and ff_gemm_pipe (update items).  A change to their stage schedule must not change a bit: the k order inside
a chunk, the chunk cuts and the order in which slabs and updates are summed are fixed, and the MFMA sequence of every
accumulator is the same.  Two references, after one iteration from a fixed state:
  * form_factor_roles_kernel (IPM_FF_REF_ENGINE=1), the same launch on the engines' previous stage schedule, in the same build;
  * tests/golden/ff_engine_factor.json: sha256 digests of the factor and the iterate recorded with that schedule.
The cases cover a dropped upper half (every pair whose upper tile lies above the diagonal), a dropped lower half and a ragged
last block (21 blocks), the top of the default size rule (72 blocks) and the chunking knob IPM_FF_Q.  Every run also checks
the factor against the serial path's (different summation order: a tolerance, not bits)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                              # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ff_engine_factor.json")

# name -> (m, n, environment of the fused run)
CASES = {
    "2048x4096": (2048, 4096, {"IPM_FUSED_FACTOR": "1"}),                  # 16 blocks
    "2048x4096_q1": (2048, 4096, {"IPM_FUSED_FACTOR": "1", "IPM_FF_Q": "1"}),
    "2048x4096_q3": (2048, 4096, {"IPM_FUSED_FACTOR": "1", "IPM_FF_Q": "3"}),
    "2048x4096_q16": (2048, 4096, {"IPM_FUSED_FACTOR": "1", "IPM_FF_Q": "16"}),
    "2600x5300": (2600, 5300, {"IPM_FUSED_FACTOR": "force"}),              # 21 blocks: lower half dropped, last block 40 rows
    "9216x18432": (9216, 18432, {"IPM_FUSED_FACTOR": "1"}),                # 72 blocks
}


def problem(m, n):
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n))
    b, c = A @ np.ones(n), A.T @ np.ones(m) + 1.0
    x, s, y = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n), rng.standard_normal(m)
    return A, b, c, (x, y, s)


def run(A, b, c, state, env):
    """One iteration on a fresh handle under `env` (restored afterwards): factor, iterate and the schedule words."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with ipm.IpmSolver(A, b, c) as sv:
            sv.set_state(*state)
            sv.iterate(1)
            x, y, s = sv.get_state()
            L = sv.get_factor()
            sch = sv.schedule()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return {"L": L, "x": x, "y": y, "s": s}, sch


def digests(r):
    return {k: hashlib.sha256(np.ascontiguousarray(r[k], dtype=np.float64).tobytes()).hexdigest() for k in ("L", "x", "y", "s")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_factor_bitwise_equal_to_reference_engines(case):
    m, n, env = CASES[case]
    with open(GOLDEN) as fh:
        want = json.load(fh)[case]
    A, b, c, state = problem(m, n)
    r, sch = run(A, b, c, state, env)
    assert sch["fused_factor"] == 1 and sch["timeouts_recovered"] == 0, sch
    assert digests(r) == want
    ref, sch_ref = run(A, b, c, state, {**env, "IPM_FF_REF_ENGINE": "1"})
    assert sch_ref["fused_factor"] == 1 and sch_ref["timeouts_recovered"] == 0, sch_ref
    for k in ("L", "x", "y", "s"):
        assert np.array_equal(r[k], ref[k]), k
    del ref
    L = r.pop("L")
    r0, sch0 = run(A, b, c, state, {"IPM_FUSED_FACTOR": "0"})
    assert sch0["fused_factor"] == 0, sch0
    rl = float(np.max(np.abs(L - r0["L"])) / np.max(np.abs(r0["L"])))
    print(f"[ff] {case}: rel L to serial {rl:.3e}")
    assert rl < 1e-10
