"""Host tests (no GPU) of the option-compatibility tables: the library's (csrc/host_compat.h, read back through ipm_debug_compat) and
the front ends' (options.ROWS).  (a) the library's table is symmetric except for the rows it declares one-directional, listed here by
name; (b) the two tables hold the same pairs with the same lifts; (c) every front end refuses every row that applies to it, with
ValueError, before the library is loaded; (d) outside the two compat units no host unit grows a ladder of its own again."""
import ctypes as C
import glob
import itertools
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, analysis, batch, batches, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "interiorpointmethod_amd")
CSRC = os.path.join(PKG, "csrc")
ERR_INVALID_ARG = -1                                    # include/ipm_hip.h: IPM_ERR_INVALID_ARG
F = {name: i for i, name in enumerate(_lib.FEATURES)}

# The rows the library declares one-directional, (a, b): switching a on beside b is refused, b beside a is not.
#   correctors / refinement x small_path: a handle that holds rounds still goes onto the small path; its solve entries refuse then
#   lockstep x bounds: ipm_set_bounds on a lockstep handle is accepted; the handle is refused where it joins a batch
#   mehrotra_start x free: an operation, nothing is held afterwards
ONE_WAY = {("correctors", "small_path"), ("refinement", "small_path"), ("lockstep", "bounds"), ("mehrotra_start", "free")}
# pairs only the library can decide (no keyword names the path before A is on the device; a bounded lockstep solver is refused by
# the library where it joins): no row of options.ROWS
LIBRARY_ONLY = {frozenset(("lockstep", "bounds"))}


def compat(a, b):
    """(excluded, lifted_by's name or None) of switching a on beside b."""
    ex, lift = C.c_int32(-7), C.c_int32(-7)
    assert ipm.load_library().ipm_debug_compat(F[a], F[b], C.byref(ex), C.byref(lift)) == _lib.IPM_OK
    assert ex.value in (0, 1) and (lift.value == -1 or ex.value == 1)
    return bool(ex.value), None if lift.value < 0 else _lib.FEATURES[lift.value]


def test_feature_ids_and_bad_arguments():
    lib = ipm.load_library()
    n = len(_lib.FEATURES)
    assert lib.ipm_debug_compat(n - 1, 0, None, None) == _lib.IPM_OK           # either pointer may be NULL
    for a, b in ((n, 0), (0, n), (-1, 0), (0, -1)):
        assert lib.ipm_debug_compat(a, b, None, None) == ERR_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "ipm_hip.h")).read()
    body = re.search(r"enum \{\s*IPM_FEATURE_BOUNDS = 0,(.*?)IPM_FEATURE_COUNT\s*\};", header, re.S).group(1)
    names = ["bounds"] + [s.strip()[len("IPM_FEATURE_"):].lower() for s in body.split(",") if s.strip()]
    assert ["quad" if nm == "quadratic" else nm for nm in names] == list(_lib.FEATURES)


def test_rows_written_out():
    """A few rows by hand, nothing of them read from either table."""
    assert compat("quad", "detect") == (True, "detect_qp") and compat("free", "detect") == (True, "detect_qp")
    assert compat("free_lp", "detect") == (True, None) and compat("free_lp", "quad") == (True, None) and compat("free", "free_lp") == (True, None)
    assert compat("quad", "small_path") == (True, "small_quadratic_flag") and compat("free", "small_path") == (True, "small_free_flag")
    assert compat("lockstep", "bounds") == (True, "lockstep_bounds") and compat("bounds", "lockstep") == (False, None)
    assert compat("correctors", "quad") == (True, None) and compat("correctors", "free") == (False, None)
    assert compat("bounds", "quad") == (False, None) and compat("refinement", "quad") == (False, None) and compat("bounds", "bounds") == (False, None)
    for x in ("quad", "free", "free_lp", "correctors", "refinement", "dense_split", "detect_qp"):
        assert compat(x, "lockstep") == (True, None), x


def test_symmetric_except_the_declared_rows():
    for a, b in itertools.product(_lib.FEATURES, repeat=2):
        if (a, b) in ONE_WAY:
            assert compat(a, b)[0] and not compat(b, a)[0], (a, b)
        elif (b, a) not in ONE_WAY:
            assert compat(a, b) == compat(b, a), (a, b)


def library_pairs():
    return {(frozenset((a, b)), compat(a, b)[1]) for a, b in itertools.product(_lib.FEATURES, repeat=2) if compat(a, b)[0]}


def test_python_and_library_tables_agree():
    lib_rows = {(p, lift) for p, lift in library_pairs() if "small_path" not in p and p not in LIBRARY_ONLY}
    py_rows = {(frozenset(r.pair), r.lifted_by) for r in options.ROWS if r.pair}
    assert py_rows == lib_rows, (sorted(map(str, py_rows - lib_rows)), sorted(map(str, lib_rows - py_rows)))
    for r in options.ROWS:                                   # every pair names two features, every lift one
        assert r.pair is None or (len(set(r.pair)) == 2 and set(r.pair) <= set(F)), r
        assert r.lifted_by is None or r.lifted_by in F, r
    for where in FRONT_ENDS:                                 # one row per pair and front end
        pairs = [frozenset(r.pair) for r in options.ROWS if r.pair and where in r.where]
        assert len(pairs) == len(set(pairs)), where
    assert len(options.ROWS) == len({(r.where, r.a, r.b) for r in options.ROWS})


# ------------------------------------------------------------------------------- (c) every front end, every row
N = 4
G = np.array([1.0, 0.0, 0.0, 0.0])
A_, B_, C_ = sparse.csc_matrix(np.eye(2, N)), np.ones(2), np.ones(N)
UB = np.array([np.inf, np.inf, np.inf, 5.0])
ON = {"quad": dict(quad=G), "free": dict(free=[0], quad=G), "free_lp": dict(free_lp=[1]), "detect_qp": dict(detect_qp=True, quad=G), "lockstep": dict(lockstep=True),
      "detect_infeasibility": dict(detect_infeasibility=True), "correctors": dict(correctors=2), "refine": dict(refine=1), "dense_cols": dict(dense_cols=[0]),
      "start": dict(start="mehrotra"), "ub": dict(ub=UB), "lockstep_bounds": dict(lockstep_bounds=True)}
FRONT_ENDS = {
    "IpmSolver": [lambda **kw: ipm.IpmSolver(A_, B_, C_, **kw)],
    "solve_with_info": [lambda **kw: ipm.solve_with_info(A_, B_, C_, **kw), lambda **kw: ipm.solve(A_, B_, C_, **kw)],
    "the lockstep batch": [lambda **kw: batches.solve_lockstep([], **kw), lambda **kw: batch.solve_shard_lockstep([], [], **kw)],
    "the small-LP batch": [lambda **kw: batches.solve_small_batch([], **kw), lambda **kw: batches.solve_small_batch_solvers([], **kw)],
    "run_batch": [lambda **kw: batch.run_batch([], **kw)],
}
CASES = [(w, i) for i, r in enumerate(options.ROWS) for w in r.where if w in FRONT_ENDS]


@pytest.mark.parametrize("where,i", CASES, ids=["%s-%s-x-%s" % (w.replace(" ", "_"), options.ROWS[i].a, options.ROWS[i].b.replace(" ", "_")) for w, i in CASES])
def test_every_front_end_refuses_every_row_before_the_library(monkeypatch, where, i):
    def boom(*a, **k):
        raise AssertionError("the library was reached before the options check refused the call")
    r = options.ROWS[i]
    kw = {r.a: ON[r.a][r.a]} if r.b in r.where else dict(ON[r.a])          # (a batch front end is its own partner)
    if r.b == "prepared":
        kw["prepared"] = analysis.prepare(A_, B_, C_)
    elif r.b not in r.where and not r.needs:
        kw.update(ON[r.b])
    monkeypatch.setattr(_lib, "load", boom)
    ran = 0
    for call in FRONT_ENDS[where]:
        try:
            with pytest.raises(ValueError) as e:
                call(**kw)
        except TypeError:                                    # this entry of the front end has no such keyword (its parameter list is pinned)
            continue
        ran += 1
        assert re.match(r"(%s)\b" % "|".join(kw), str(e.value)) or "Prepared" in str(e.value), str(e.value)
    assert ran
    if r.text is None and where in ("the lockstep batch", "the small-LP batch", "run_batch"):          # a batch row alone: its own words
        with pytest.raises(ValueError, match=re.escape(r.why) if r.why else re.escape(where)):
            FRONT_ENDS[where][0](**kw)


def test_lifts_and_clears_are_accepted_by_the_options_check():
    for r in options.ROWS:
        if r.lifted_by:
            kw = dict(ON[r.a], **ON[r.b])
            with pytest.raises(ValueError):
                options.check_options("IpmSolver", N, **kw)
            options.check_options("IpmSolver", N, **dict(kw, **ON[r.lifted_by]))
    v = options.check_options("IpmSolver", N, quad=np.zeros(N), free=[], free_lp=np.zeros(N, dtype=bool), lockstep=True, correctors=0, detect_infeasibility=True)
    assert v["quad"] is None and v["free"] is None and v["free_lp"] is None and v["correctors"] == 0
    options.check_options("IpmSolver", N, lockstep_bounds=True, lockstep=True)


# ------------------------------------------------------------------------------- (d) no ladder outside the compat units
# what the ladders looked like: `if (h->lockstep) return fail(...)`, `if (h->detect && !h->detect_qp) return fail(`, `if (h->quad) return fail(`,
# `if (h->mcc.k > 0) return fail(`, `if (h->free_on) return fail(` (now a ColumnSet's `on`), also through hs[i]-> in the batch entries
LADDER = re.compile(r"(?:\bh|\bhs\[\w+\])->(?:lockstep\b|detect\w*\b|quad\b|mcc\.k\b|\w+\.on\b)")


def test_the_ladder_pattern_knows_the_ladders():
    for line in ('if (h->lockstep) return fail(h, IPM_ERR_INVALID_ARG, "x");', 'if (h->detect && !h->detect_qp) return fail(h, 1, "x");',
                 'if (h && h->quad && k > 0) return fail(h, 1, "x");', 'if (h->mcc.k > 0) return fail(h, 1, "%d", h->mcc.k);',
                 'if (hs[i]->free_set.on) return fail(nullptr, 1, "x");', 'if (h->free_lp_set.on) return fail(h, 1, "x");'):
        assert LADDER.search(line), line
    for line in ('if (!h->small) return fail(nullptr, 1, "x");', 'if (h->quad_nnz) x();', 'if (rounds_on(r)) return fail(h, 1, "x");'):
        assert not LADDER.search(line), line


def test_host_units_hold_no_option_ladder():
    files = sorted(glob.glob(os.path.join(CSRC, "host_*.h"))) + [os.path.join(CSRC, "ipm_api.hip")]
    assert len(files) >= 11 and os.path.join(CSRC, "host_compat.h") in files
    hits = []
    for path in files:
        if os.path.basename(path) == "host_compat.h":
            continue
        for no, line in enumerate(open(path), 1):
            code = line.split("//")[0]
            if "return fail(" in code and LADDER.search(code.split("return fail(")[0]):
                hits.append("%s:%d: %s" % (os.path.basename(path), no, code.strip()[:120]))
    assert not hits, "an option exclusion tested outside host_compat.h:\n" + "\n".join(hits)


def test_python_modules_call_no_refusal_of_their_own():
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) >= 10
    hits = []
    for path in files:
        if os.path.basename(path) == "options.py":
            continue
        for no, line in enumerate(open(path), 1):
            if re.search(r"\brefuse_\w+\(", line.split("#")[0]) and not line.lstrip().startswith("def "):
                hits.append("%s:%d: %s" % (os.path.basename(path), no, line.strip()[:120]))
    assert not hits, "a refuse_* call outside options.py:\n" + "\n".join(hits)
