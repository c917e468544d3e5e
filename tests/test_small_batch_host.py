"""The small-LP batch (ipm_solve_small_batch, solver.solve_small_batch) on a host without a GPU: the symbol is declared, exported and
bound; the argument checks that need no device answer with a message; the Python entry point refuses an LP of more than 128 rows
before it creates a handle.  The device side is tests/test_gpu_small_batch.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_exported_and_bound(built_lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipm_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+ipm_solve_small_batch\s*\(([^)]*)\)", txt)
    assert decl, "include/ipm_hip.h does not declare ipm_solve_small_batch"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("ipm_handle**") and args[6].startswith("void*") and args[7].startswith("ipm_stats*")
    assert hasattr(C.CDLL(built_lib), "ipm_solve_small_batch")
    assert "ipm_solve_small_batch" in _lib.EXPORTS
    assert re.search(r"#define\s+IPM_ABI_VERSION\s+4\b", txt)          # additive: the ABI version stays
    for name in ("solve_small_batch", "solve_small_batch_solvers", "small_batch_eligible"):
        assert hasattr(ipm, name) and name in ipm.__all__


def test_empty_batch_is_ok_without_a_device(built_lib):
    lib = ipm.load_library()
    assert lib.ipm_solve_small_batch(None, 0, 1e-8, 1e-8, 1e-8, 100, None, None) == 0
    hs = (C.c_void_p * 1)(None)
    assert lib.ipm_solve_small_batch(hs, 0, 1e-8, 1e-8, 1e-8, 100, None, None) == 0
    assert ipm.solve_small_batch_solvers([]) == []
    assert ipm.solve_small_batch([]) == []


def test_bad_arguments_answer_with_a_message(built_lib):
    lib = ipm.load_library()
    assert lib.ipm_solve_small_batch(None, -1, 1e-8, 1e-8, 1e-8, 100, None, None) == -1
    assert b"n = -1" in lib.ipm_last_error(None)
    assert lib.ipm_solve_small_batch(None, 3, 1e-8, 1e-8, 1e-8, 100, None, None) == -1
    assert b"handles is NULL" in lib.ipm_last_error(None)
    hs = (C.c_void_p * 1)(None)
    assert lib.ipm_solve_small_batch(hs, 1, 1e-8, 1e-8, 1e-8, 100, None, None) == -1
    assert b"handle 0 is NULL" in lib.ipm_last_error(None)


def test_more_than_128_rows_is_refused_on_the_host(monkeypatch):
    """The host check runs before any handle exists: IpmSolver is never constructed."""
    def no_device(*a, **k):
        raise AssertionError("a handle was created before the host check refused the batch")
    monkeypatch.setattr(batches, "IpmSolver", no_device)
    rng = np.random.default_rng(0)
    ok = (sparse.random(20, 40, density=0.3, random_state=1, format="csc") + sparse.eye(20, 40, format="csc"), np.ones(20), np.ones(40))
    big = (rng.standard_normal((129, 300)), np.ones(129), np.ones(300))
    with pytest.raises(ValueError, match="problem 1 has 129 rows"):
        ipm.solve_small_batch([ok, big])
    with pytest.raises(ValueError, match="problem 0 has 129 rows"):
        ipm.solve_small_batch([big, ok])
    with pytest.raises(ValueError, match="one per problem"):
        ipm.solve_small_batch([ok, ok], ub=[None])
    with pytest.raises(ValueError, match="problem 1: ub has negative entries"):
        ipm.solve_small_batch([ok, ok], ub=[None, -np.ones(40)])
