"""Host side of the bounded twins of the lockstep batch (IPM_FLAG_LOCKSTEP_BOUNDS): no GPU.

  * the header: the eight bounded kernel types continue enum LsType of csrc/lockstep.h in a declaration of their own (the old block
    keeps the text tests/lockstep_wide_cases.py restates), and the flag is bit 7, alone on its bit;
  * the schedule merge (ipm_debug_ls_merge) over programs in which half of the members run the bounded vector types;
  * batch.unpack_problem, the one statement of the (A, b, c) / (A, b, c, ub) rule, and the front ends that unpack through it;
  * general_form.native_problem against native_form.
"""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batch
from interiorpointmethod_amd import general_form as G

import lockstep_wide_cases as W
from test_lockstep_merge import check, merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "general")

# the bounded twin of each plain vector type, by name (enum LsBndType of csrc/lockstep.h)
BND_NAMES = ("PREPARE_BND", "PREPARE_DETECT_BND", "STOP_TEST_BND", "STOP_TEST_DETECT_BND", "DIRECTION_BND", "MU_AFF_BND", "CORR_RHS_BND",
             "UPDATE_BND")
PLAIN_VECTOR = ("PREPARE", "STOP_TEST", "DIRECTION", "MU_AFF", "CORR_RHS", "UPDATE")          # the six plain steps a bounded LP replaces


def _header():
    return open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "lockstep.h")).read()


def bounded_ids():
    """name -> id of the bounded types, parsed from csrc/lockstep.h (shared with tests/test_gpu_lockstep_bounds.py)."""
    body = re.search(r"enum LsBndType \{(.*?)\};", _header(), re.S).group(1)
    names = [t.strip() for t in body.replace("\n", " ").split(",")]
    assert names[0] == "LS_PREPARE_BND = LS_NTYPES" and names[-1] == "LS_NTYPES_ALL"
    names[0] = "LS_PREPARE_BND"
    return {nm[len("LS_"):]: len(W.LS_TYPES) + k for k, nm in enumerate(names[:-1])}


# ---- 1. the header ------------------------------------------------------------------------------------------------------------
def test_bounded_types_continue_the_old_enum():
    txt = _header()
    old = re.search(r"enum LsType \{(.*?)\};", txt, re.S).group(1)
    names = [t.strip() for t in old.replace("\n", " ").split(",")]
    assert names[0] == "LS_SPMV_CSR = 0" and names[-1] == "LS_NTYPES"
    assert tuple(n.replace(" = 0", "")[len("LS_"):] for n in names[:-1]) == W.LS_TYPES          # the old block, name by name
    ids = bounded_ids()
    assert tuple(ids) == BND_NAMES and len(ids) == 8
    assert sorted(ids.values()) == list(range(len(W.LS_TYPES), len(W.LS_TYPES) + 8))           # from LS_NTYPES on, contiguous
    for nm in PLAIN_VECTOR + ("PREPARE_DETECT", "STOP_TEST_DETECT"):
        assert nm + "_BND" in ids and nm in W.LS
    # every new type has its twin declaration and its wrapper, and the launch table spans the new total
    for nm in BND_NAMES:
        assert len(re.findall(r"struct LsTwin<LS_%s>" % nm, txt)) == 1 and len(re.findall(r"LS_KERNEL\(LS_%s," % nm, txt)) == 1
    assert "make_integer_sequence<int, LS_NTYPES_ALL>" in txt and "type >= LS_NTYPES_ALL" in txt


def test_flag_is_bit_seven_and_alone():
    txt = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"\b(IPM_FLAG_[A-Z_]+)\s*=\s*(\d+)", txt)}
    # the new enumerator is written as the bit after the last one (the list of literal values above stays what it was)
    m = re.search(r"\bIPM_FLAG_LOCKSTEP_BOUNDS\s*=\s*(IPM_FLAG_[A-Z_]+)\s*<<\s*(\d+)", txt)
    assert m and "IPM_FLAG_LOCKSTEP_BOUNDS" not in flags
    value = flags[m.group(1)] << int(m.group(2))
    assert value == 128 == _lib.FLAG_LOCKSTEP_BOUNDS
    assert all(v & value == 0 for v in flags.values())
    mine = {k: v for k, v in vars(_lib).items() if k.startswith("FLAG_")}
    assert [k for k, v in mine.items() if v & 128] == ["FLAG_LOCKSTEP_BOUNDS"]
    assert set(mine) == {k[len("IPM_"):] for k in flags} | {"FLAG_LOCKSTEP_BOUNDS"}
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt) and _lib.ABI_VERSION == 4      # additive: the ABI version stays
    # the library's own statement of the value (a static_assert next to the check in ipm_create)
    api = open(os.path.join(ROOT, "interiorpointmethod_amd", "csrc", "ipm_api.hip")).read()
    assert "static_assert(IPM_FLAG_LOCKSTEP_BOUNDS == 128" in api


def test_python_keyword_and_its_refusal():
    p = inspect.signature(ipm.IpmSolver.__init__).parameters
    assert p["lockstep_bounds"].default is False
    A = sparse.csc_matrix(np.eye(3))
    with pytest.raises(ValueError, match="lockstep=True"):          # before any device is touched
        ipm.IpmSolver(A, np.ones(3), np.ones(3), lockstep_bounds=True)


# ---- 2. the merge --------------------------------------------------------------------------------------------------------------
FAMILY_TEMPLATES = {"two": (2, "group"), "three": (3, "block"), "six": (6, "group")}


def _bounded(prog, ids):
    swap = {W.LS[nm]: ids[nm + "_BND"] for nm in PLAIN_VECTOR}
    return [swap.get(t, t) for t in prog]


def _programs(families, members, ids):
    """`members` programs, the families cycling; every second member runs the bounded vector types."""
    plain = [W.template(*FAMILY_TEMPLATES[families[i % len(families)]]) for i in range(members)]
    return plain, [_bounded(p, ids) if i % 2 else p for i, p in enumerate(plain)]


@pytest.mark.parametrize("aligned", [1, 0], ids=["aligned", "leader"])
@pytest.mark.parametrize("members", [2, 64, 65])
@pytest.mark.parametrize("families", [("two",), ("three",), ("six",), ("two", "three", "six")], ids=["two", "three", "six", "mixed"])
def test_merge_with_bounded_members(families, members, aligned):
    ids = bounded_ids()
    plain, mixed = _programs(families, members, ids)
    per_program = sum(1 for t in mixed[1] if t in ids.values())
    assert per_program == 7 and set(t for t in mixed[1] if t >= len(W.LS_TYPES)) == {ids[nm + "_BND"] for nm in PLAIN_VECTOR}
    plan = merge(mixed, max_group=W.LS_MAX_GROUP, aligned=aligned)
    check(mixed, plan, W.LS_MAX_GROUP)                   # every program's order kept, one id per step, at most 64 members
    base = merge(plain, max_group=W.LS_MAX_GROUP, aligned=aligned)
    check(plain, base, W.LS_MAX_GROUP)
    print("OBS merge %s x %d %s: %d steps, all-unbounded %d" % ("+".join(families), members, "aligned" if aligned else "leader", len(plan), len(base)))
    # The step bound is asserted for every family under both rules, and for the families mixed under the progressive alignment, the
    # merge a batch runs.  The leader rule (IPM_LS_MERGE=leader, kept for the A/B) already loses steps on out-of-phase programs
    # without any bounded member (test_lockstep_merge.test_out_of_phase_programs); mixed families with bounded members gave 80
    # steps against 70 at 64 members and 50 against 45 at 2: its order and one-id-per-step properties are held above, no step bound.
    if aligned or len(families) == 1:
        assert len(plan) <= len(base) + per_program


# ---- 3. the tuple rule ---------------------------------------------------------------------------------------------------------
def _tiny():
    A = sparse.csc_matrix(np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 1.0]]))
    return A, np.ones(2), np.ones(3)


def test_unpack_problem():
    A, b, c = _tiny()
    t3 = batch.unpack_problem((A, b, c))
    t4 = batch.unpack_problem((A, b, c, None))
    tinf = batch.unpack_problem((A, b, c, np.full(3, np.inf)))
    for t in (t3, t4, tinf):
        assert len(t) == 4 and t[0] is A and t[1] is b and t[2] is c and t[3] is None
    u = np.array([np.inf, 2.0, np.inf])
    got = batch.unpack_problem((A, b, c, [np.inf, 2, np.inf]))[3]
    assert got.dtype == np.float64 and np.array_equal(got, u)
    for bad in (np.ones(2), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0])):
        with pytest.raises(ValueError):
            batch.unpack_problem((A, b, c, bad))
    for n in (2, 5):
        with pytest.raises(ValueError, match="a problem is"):
            batch.unpack_problem((A, b, c, None, None)[:n])


def test_front_ends_check_ub_before_any_device_work(monkeypatch):
    """No GPU here: a front end that touched the device before the check would raise something else than ValueError."""
    A, b, c = _tiny()

    def boom(*a, **k):
        raise AssertionError("device work before the host check")

    monkeypatch.setattr(batch, "solve_with_info", boom)
    monkeypatch.setattr(batch, "IpmSolver", boom)
    monkeypatch.setattr(batch, "prepare", boom)
    for bad in (np.ones(2), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0])):
        probs = [(A, b, c), (A, b, c, bad)]
        with pytest.raises(ValueError):
            batch.solve_one(probs[1])
        with pytest.raises(ValueError):
            batch.solve_shard(probs, [0, 1])
        with pytest.raises(ValueError):
            batch.solve_shard_lockstep(probs, [0, 1])
        for lockstep in (False, True):
            with pytest.raises(ValueError):
                batch.run_batch(probs, workers=2, lockstep=lockstep)


def test_lockstep_wanted_and_predicted_cost_take_both_forms():
    A = sparse.csc_matrix((300, 400))
    u = np.full(400, 2.0)
    for p in ((A, None, None), (A, None, None, None), (A, None, None, u)):
        assert batch.predicted_cost(p) == batch.predicted_cost(300, 400)
        assert batch.lockstep_wanted([p] * batch.LOCKSTEP_MIN_LPS, workers=8, mode="auto")
        assert not batch.lockstep_wanted([p] * (batch.LOCKSTEP_MIN_LPS - 1), workers=8, mode="auto")
        assert batch.lockstep_wanted([p], workers=8, mode=True) and not batch.lockstep_wanted([p], workers=1, mode=True)
    with pytest.raises(ValueError):
        batch.lockstep_wanted([(A, None, None, np.ones(3))], mode="auto")
    with pytest.raises(ValueError):
        batch.predicted_cost((A, None, None, -u))
    # a custom solve_fn still receives its problems as they are
    seen = []
    rec, _ = batch.run_batch([(A, "b", "c", "anything")], solve_fn=lambda p, device=0, **kw: (seen.append(p), dict(batch._error_info(1.0)))[1])
    assert seen[0][3] == "anything" and rec[0, 1] == 1.0


# ---- 4. native_problem ---------------------------------------------------------------------------------------------------------
def _load_general(name):
    z = np.load(os.path.join(GEN, name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


@pytest.mark.parametrize("name,bounds", [("GROW7", 280), ("AFIRO", 0)])
def test_native_problem_equals_native_form(name, bounds):
    args = _load_general(name)
    F0 = G.native_form(**args)
    (A, b, c, u), F = G.native_problem(**args)
    assert isinstance(F, G.NativeForm) and A is F.A and b is F.b and c is F.c and u is F.u
    for f in G.NativeForm.__slots__:
        a, a0 = getattr(F, f), getattr(F0, f)
        if sparse.issparse(a):
            assert a.shape == a0.shape and (a != a0).nnz == 0, f
        else:
            assert np.array_equal(np.asarray(a), np.asarray(a0)), f
    assert int(np.isfinite(u).sum()) == bounds
    A4, b4, c4, u4 = batch.unpack_problem((A, b, c, u))          # ... and it is a problem of the batched-LP mode
    assert (u4 is None) == (bounds == 0)
