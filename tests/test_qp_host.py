"""The host side of the separable convex QP (ipm_set_quadratic): what holds without a device -- the symbols, the
keyword in every signature that takes it, the host checks of the diagonal and the refusals that are decided before a device is
touched.  The refusals the library itself decides are in tests/test_gpu_qp.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ipm_set_quadratic", "ipm_get_quadratic")


def test_symbols_in_header_binding_and_library(built_lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipm_hip.h")).read(), flags=re.S)
    lib = C.CDLL(built_lib)
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\s*\(ipm_handle\* h, " % sym, txt), sym
        assert sym in _lib.EXPORTS and hasattr(lib, sym), sym
    assert _lib.ABI_VERSION == 4 and lib.ipm_abi_version() == 4          # additive: no version bump


def test_null_handle_is_an_argument_error(built_lib):
    lib = ipm.load_library()
    g = np.ones(3)
    assert lib.ipm_set_quadratic(None, g.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert b"ipm_set_quadratic" in lib.ipm_last_error(None)
    assert lib.ipm_get_quadratic(None, None, None) == -1


@pytest.mark.parametrize("fn", [ipm.solve, ipm.solve_with_info, ipm.interior_sparse, ipm.IpmSolver.__init__])
def test_quad_keyword_in_the_signatures(fn):
    p = inspect.signature(fn).parameters
    assert "quad" in p and p["quad"].default is None


@pytest.mark.parametrize("fn", [ipm.new_interior_sparse, ipm.solve_lockstep, ipm.solve_small_batch])
def test_front_ends_that_do_not_take_it(fn):
    assert "quad" not in inspect.signature(fn).parameters


def test_check_quadratic():
    assert handle.check_quadratic(None, 4) is None
    assert handle.check_quadratic(np.zeros(4), 4) is None                 # all zeros: the LP
    g = handle.check_quadratic([0, 1, 2.5, 0], 4)
    assert g.dtype == np.float64 and g.tolist() == [0.0, 1.0, 2.5, 0.0]
    assert handle.check_quadratic(np.ones((4, 1)), 4).shape == (4,)
    for bad in ([1.0, 2.0, 3.0], np.ones(5), [1, np.nan, 0, 0], [1, np.inf, 0, 0], [1, -1e-300, 0, 0]):
        with pytest.raises(ValueError, match="quad"):
            handle.check_quadratic(bad, 4)


A, b, c = np.ones((2, 4)), np.ones(2), np.ones(4)
G = np.array([1.0, 0.0, 2.0, 0.0])


@pytest.mark.parametrize("kw", [dict(lockstep=True), dict(detect_infeasibility=True), dict(correctors=1)], ids=lambda kw: next(iter(kw)))
def test_solver_refuses_before_a_device_is_touched(kw):
    with pytest.raises(ValueError, match="quad"):
        ipm.IpmSolver(A, b, c, quad=G, **kw)


@pytest.mark.parametrize("kw", [dict(detect_infeasibility=True), dict(correctors=2)], ids=lambda kw: next(iter(kw)))
def test_solve_refuses_before_a_device_is_touched(kw):
    for fn in (ipm.solve, ipm.solve_with_info):
        with pytest.raises(ValueError, match="quad"):
            fn(A, b, c, quad=G, **kw)
    with pytest.raises(ValueError, match="quad"):
        ipm.interior_sparse(A, b, c, quad=G, **kw)


def test_wrong_values_raise_before_a_device_is_touched():
    for bad in (np.ones(3), [1, np.nan, 0, 0], [1, -1, 0, 0], [np.inf, 0, 0, 0]):
        with pytest.raises(ValueError, match="quad"):
            ipm.IpmSolver(A, b, c, quad=bad)
        with pytest.raises(ValueError, match="quad"):
            ipm.solve(A, b, c, quad=bad)
