"""The device Mehrotra start on a host without a GPU: the two symbols are declared and exported, the ABI version stays, the argument
checks that need no device, the front end's start keyword and the 5 % rule (handle.wants_shift)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, api, batch, batches, handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipm_hip.h")


def test_header_and_exports(built_lib):
    txt = open(HEADER).read()
    for name, args in (("ipm_init_state_mehrotra", ["ipm_handle*", "int32_t*"]),
                       ("ipm_init_small_batch_mehrotra", ["ipm_handle**", "int32_t", "void*", "int32_t*"])):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
        assert decl, "include/ipm_hip.h does not declare %s" % name
        types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in decl.group(1).split(",")]
        assert types == args, (name, types)
        assert hasattr(C.CDLL(built_lib), name) and name in _lib.EXPORTS
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt) and _lib.ABI_VERSION == 4
    assert "init_small_batch_mehrotra" in ipm.__all__ and ipm.init_small_batch_mehrotra is batches.init_small_batch_mehrotra
    assert hasattr(ipm.IpmSolver, "init_state_mehrotra")


def test_argument_checks_without_a_device(built_lib):
    lib = _lib.load()
    assert lib.ipm_init_state_mehrotra(None, None) == -1 and b"NULL handle" in lib.ipm_last_error(None)
    assert lib.ipm_init_small_batch_mehrotra(None, 0, None, None) == 0          # n == 0: IPM_OK, no device touched
    hs = (C.c_void_p * 1)(None)
    assert lib.ipm_init_small_batch_mehrotra(hs, 0, None, None) == 0
    assert lib.ipm_init_small_batch_mehrotra(None, -1, None, None) == -1
    assert lib.ipm_init_small_batch_mehrotra(None, 3, None, None) == -1
    assert lib.ipm_init_small_batch_mehrotra(hs, 1, None, None) == -1 and b"handle 0 is NULL" in lib.ipm_last_error(None)


def test_bogus_start_is_refused_before_any_handle(monkeypatch):
    made = []
    monkeypatch.setattr(batches, "IpmSolver", lambda *a, **k: made.append(1))
    monkeypatch.setattr(api, "IpmSolver", lambda *a, **k: made.append(1))
    A = np.array([[1.0, 2.0]])
    with pytest.raises(ValueError, match="start"):
        ipm.solve_small_batch([(A, np.ones(1), np.ones(2))], start="bogus")
    with pytest.raises(ValueError, match="start"):
        ipm.solve_with_info(A, np.ones(1), np.ones(2), start="bogus", device_start=True)
    with pytest.raises(ValueError, match="start"):
        batch.solve_shard_lockstep([(A, np.ones(1), np.ones(2))], [0], start="bogus")
    assert not made


def test_five_percent_rule():
    """The decisions the inline rule of solve_with_info took: pivots_fixed > 0.05 m, only with no shift asked for and the automatic
    shift allowed."""
    w = handle.wants_shift
    assert not w(5, 100) and w(6, 100) and not w(4, 100) and not w(0, 100)          # at 5 % exactly: no
    assert not w(1, 20) and w(2, 20) and w(1, 19)
    assert not w(50, 100, regularize=1e-10) and not w(50, 100, auto_regularize=False)
    assert w(50, 100, regularize=0.0) and w(50, 100, regularize=None)
    for fixed in range(0, 40):
        for m in (1, 19, 20, 21, 128, 205):
            assert w(fixed, m) == (fixed > 0.05 * m)
    assert handle.shift_allowed() and not handle.shift_allowed(1e-14) and not handle.shift_allowed(0.0, False)


def test_run_batch_passes_start_to_the_lockstep_shard(monkeypatch):
    """run_batch no longer drops `start` on the lockstep path."""
    seen = {}

    def fake(problems, ids, **kw):
        seen.update(kw)
        return np.zeros((len(ids), batch.NF))
    monkeypatch.setattr(batch, "solve_shard_lockstep", fake)
    A = np.ones((200, 3))
    batch.run_batch([(A, None, None)], workers=2, lockstep=True, start="mehrotra")
    assert seen.get("start") == "mehrotra"
