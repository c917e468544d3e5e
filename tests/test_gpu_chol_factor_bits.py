"""GPU test (-m gpu): the dense blocked Cholesky that enqueue_factor runs (csrc/host_factor_solve.h, step plan: csrc/chol_plan.h),
pinned bit for bit.  tests/golden/chol_factor_digests.json holds sha256 digests recorded on an MI355X with the library built from
the commit the file names: the last one in which enqueue_factor decided its schedule while it launched.  The plan is a restatement of
that schedule, so every launch, argument, stream and hand-off is the same and no bit of any result may move.

Cases: the smallest shapes that reach each branch of the plan (tests/test_chol_plan_host.py checks the plans themselves on the CPU).
  factor cases   B = M M^T + I with M of 64 seeded columns, solve_linear + get_factor; each factor is also checked against
                 np.linalg.cholesky, max |L - L_ref| <= 1e-11 max |L_ref|, so a wrong fixture cannot hide a wrong factor;
  envelope       two cases of sparse_front_cases.ENVELOPES whose envelope flag is 1: the factor after normal_solve (two_groups2048: a
                 column with nothing below its diagonal block and columns of one block; ragged2304: columns of two blocks);
  hooks          a dense LP of 16 blocks without the fused launch: (x, y, s) after iterate(2) -- the residual stream and the group
                 inverses start inside the factorization, at their steps;
  lockstep       the smallest eligible pair of tests/test_gpu_lockstep.py (SC205, E226): the states after one ipm_batch_step, i.e.
                 the factorization as a recorded program.

Recording (on the build of the commit to pin):  python tests/test_gpu_chol_factor_bits.py OUT.json COMMIT  computes every digest
twice and writes the file only if both passes agree."""
import contextlib
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import interiorpointmethod_amd as ipm                              # noqa: E402
from interiorpointmethod_amd.matio import load_npz_problem         # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp         # noqa: E402

import sparse_front_cases as FC                                    # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "chol_factor_digests.json")
KNOBS = ("IPM_GROUP_STEPS", "IPM_FLAG_SYNC", "IPM_LOOKAHEAD", "IPM_TWO_LEVEL", "IPM_BULK_VARIANT", "IPM_FUSED_FACTOR", "IPM_ENVELOPE",
         "IPM_GROUPED_TRSV", "IPM_RAGGED_GROUPS", "IPM_LIST_FORM", "IPM_FUSED_SMALL", "IPM_POTRF_STAMPS", "IPM_STREAM_AT")

# name -> (m, switches, what schedule() must report: the branch the case is there for)
FACTOR_CASES = {
    "m300": (300, {}, dict(blocks=3, group_steps=1, device_polling=1)),
    "m1100_gs1": (1100, {"IPM_GROUP_STEPS": "1"}, dict(blocks=9, group_steps=1)),
    "m1100_gs2": (1100, {"IPM_GROUP_STEPS": "2"}, dict(blocks=9, group_steps=2)),
    "m1100_gs3": (1100, {"IPM_GROUP_STEPS": "3"}, dict(blocks=9, group_steps=3)),
    "m1100_gs4": (1100, {"IPM_GROUP_STEPS": "4"}, dict(blocks=9, group_steps=4)),
    "m1100_gs3_events": (1100, {"IPM_GROUP_STEPS": "3", "IPM_FLAG_SYNC": "0"}, dict(blocks=9, group_steps=3, device_polling=0, counter_steps=0)),
    "m1100_single_stream": (1100, {"IPM_LOOKAHEAD": "0"}, dict(blocks=9, group_steps=1, counter_steps=0, event_steps=0)),
    "m2200_single_stream": (2200, {"IPM_LOOKAHEAD": "0"}, dict(blocks=18, group_steps=1, counter_steps=0, event_steps=0)),
    "m6272": (6272, {}, dict(blocks=49, group_steps=3, device_polling=1)),
}
ENVELOPE_CASES = ("two_groups2048", "ragged2304")
LOCKSTEP_PAIR = ("SC205", "E226")


@contextlib.contextmanager
def switches(env):
    """The process environment with exactly these IPM_* switches of the factorization (a handle reads them when it is created)."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def spd(m):
    """(B, rhs, np.linalg.cholesky(B)) of the factor cases with m rows, computed once and read-only."""
    rng = np.random.default_rng(4000 + m)
    M = rng.standard_normal((m, 64))
    B = M @ M.T + np.eye(m)
    rhs = rng.standard_normal(m)
    ref = np.linalg.cholesky(B)
    for a in (B, rhs, ref):
        a.setflags(write=False)
    return B, rhs, ref


def factor_case(name):
    m, env, _ = FACTOR_CASES[name]
    B, rhs, _ = spd(m)
    with switches(env):
        with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
            z, nfix = sv.solve_linear(B, rhs)
            return sv.get_factor(), z, nfix, sv.schedule()


def envelope_case(name):
    A = FC.as_float(FC.envelope_case(name))
    m, n = A.shape
    d = FC.solve_d(n, 81)
    rhs = np.random.default_rng(82).standard_normal(m)
    with switches({}):
        with ipm.IpmSolver(A, np.zeros(m), np.zeros(n), factor="dense", reorder=None) as sv:
            z = sv.normal_solve(rhs, d)
            return sv.get_factor(), z, sv.schedule()


def hooks_case():
    A, b, c = synthetic_lp(2048, 2500, seed=7)
    with switches({"IPM_FUSED_FACTOR": "0"}):
        with ipm.IpmSolver(A, b, c) as sv:
            sv.init_state(0.0)
            st = sv.iterate(2)
            return sv.get_state(), st, sv.schedule()


def lockstep_case():
    probs = []
    for nm in LOCKSTEP_PAIR:
        A, b, c, _, valid = load_npz_problem(os.path.join(HERE, "golden", "netlib", nm + ".npz"))
        assert valid
        probs.append((A, b, c))
    with switches({}):
        svs = [ipm.IpmSolver(*p, lockstep=True, factor="dense") for p in probs]
        try:
            for sv in svs:
                assert ipm.lockstep_eligible(sv)
                sv.init_state(1.0)
            with ipm.LockstepBatch(tol=1e-8, max_iter=300) as bt:
                for sv in svs:
                    bt.add(sv)
                bt.step()
            return [a for sv in svs for a in sv.get_state()]
        finally:
            for sv in svs:
                sv.close()


def all_digests():
    out = {}
    for name in sorted(FACTOR_CASES):
        L = factor_case(name)[0]
        ref = spd(FACTOR_CASES[name][0])[2]
        print("FIGURE %s: max |L - L_ref| / max |L_ref| = %.3e" % (name, float(np.max(np.abs(L - ref))) / float(np.max(np.abs(ref)))), flush=True)
        out[name] = digest(L)
    for name in ENVELOPE_CASES:
        out["envelope_" + name] = digest(envelope_case(name)[0])
    out["hooks_2048x2500"] = digest(*hooks_case()[0])
    out["lockstep_" + "_".join(LOCKSTEP_PAIR)] = digest(*lockstep_case())
    return out


def recorded(name):
    with open(GOLDEN) as fh:
        return json.load(fh)["digests"][name]


@pytest.mark.parametrize("name", sorted(FACTOR_CASES))
def test_factor_bits_are_the_recorded_ones(name):
    m, _, want_schedule = FACTOR_CASES[name]
    L, z, nfix, sch = factor_case(name)
    _, _, ref = spd(m)
    err = float(np.max(np.abs(L - ref))) / float(np.max(np.abs(ref)))
    print("FIGURE %s: max |L - L_ref| / max |L_ref| = %.3e (bound 1e-11); schedule %s" % (name, err, sch))
    assert nfix == 0 and sch["timeouts_recovered"] == 0
    for k, v in want_schedule.items():
        assert sch[k] == v, (k, sch)
    if name == "m6272":                                  # bulk updates on both sides of the 1024-workgroup rule
        assert sch["counter_steps"] > 0 and sch["event_steps"] > 0, sch
    assert err <= 1e-11
    assert digest(L) == recorded(name)


@pytest.mark.parametrize("name", ENVELOPE_CASES)
def test_envelope_factor_bits_are_the_recorded_ones(name):
    assert FC.ENVELOPES[name][2] == 1
    L, z, sch = envelope_case(name)
    assert sch["envelope"] == 1 and sch["group_steps"] == 1 and sch["timeouts_recovered"] == 0, sch
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(z))
    assert digest(L) == recorded("envelope_" + name)


def test_iterates_with_the_hooks_inside_the_factorization_are_the_recorded_ones():
    (x, y, s), st, sch = hooks_case()
    assert sch["blocks"] == 16 and sch["fused_factor"] == 0 and sch["grouped_trsv"] == 1 and sch["timeouts_recovered"] == 0, sch
    assert st["iterations"] == 2
    assert digest(x, y, s) == recorded("hooks_2048x2500")


def test_one_lockstep_step_is_the_recorded_one():
    assert digest(*lockstep_case()) == recorded("lockstep_" + "_".join(LOCKSTEP_PAIR))


if __name__ == "__main__":
    out_path, commit = sys.argv[1], sys.argv[2]
    first = all_digests()
    second = all_digests()
    for k in sorted(first):
        print(k, first[k], "same" if second[k] == first[k] else "DIFFERS " + second[k], flush=True)
    if first != second:
        sys.exit("the two passes disagree: nothing written")
    with open(out_path, "w") as fh:
        json.dump({"recorded_with": commit, "device": "MI355X", "digests": first}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path)
