"""GPU tests of the library's option-compatibility table on LIVE handles (csrc/host_compat.h): for every ordered pair the
table excludes -- read from ipm_debug_compat, so a later row is covered without an edit here, or fails for want of a recipe -- a
handle that holds the second feature is built on the smallest LP that can hold both, the first is switched on, and the call returns
IPM_ERR_INVALID_ARG with the entry point's name in the message, the handle keeps what it held (by getter), and a solve of the surviving
configuration converges.  With the row's lifting flag set the same call is accepted.  Both call orders of a pair are two ordered pairs.

The multi-kernel rows use a dense 3 x 6 LP (a finite bound on column 0, g > 0 on column 1, column 1 the free set with curvature, column
2 the LP free set), the small-path rows the same LP as a sparse matrix, which goes onto the one-workgroup path, the lockstep rows
lockstep=True.  A feature fixed at ipm_create (lockstep, detect, detect_qp) cannot be switched on later: that order does not exist;
the small path is switched on by ipm_set_A_csc, which declines it instead of refusing."""
import ctypes as C
import itertools

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = -1
FEATURES = _lib.FEATURES
F = {name: i for i, name in enumerate(FEATURES)}
A_ = np.array([[2.0, 1, 1, 1, 0, 0], [1, 3, 1, 0, 1, 0], [1, 1, 2, 0, 0, 1]])
B_ = A_ @ np.ones(6)
C_ = np.array([1.0, 2, 1, 6, 6, 6])          # (bounded below with column 2 free: y = (0, 0, 1/2) is dual feasible)
G = np.array([0.0, 0.5, 0, 0, 0, 0])
UB = np.array([4.0, np.inf, np.inf, np.inf, np.inf, np.inf])
FREE, FREE_LP = np.array([1], dtype=np.int32), np.array([2], dtype=np.int32)


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def compat(a, b):
    ex, lift = C.c_int32(0), C.c_int32(-1)
    assert ipm.load_library().ipm_debug_compat(F[a], F[b], C.byref(ex), C.byref(lift)) == 0
    return bool(ex.value), None if lift.value < 0 else FEATURES[lift.value]


# how a live handle is asked to switch a feature on: (entry point, call) -- the features a setter or an operation switches on
SWITCH = {
    "quad": ("ipm_set_quadratic", lambda sv: sv._lib.ipm_set_quadratic(sv._h, _dptr(G))),
    "free": ("ipm_set_free_columns", lambda sv: sv._lib.ipm_set_free_columns(sv._h, _iptr(FREE), 1)),
    "free_lp": ("ipm_set_free_lp_columns", lambda sv: sv._lib.ipm_set_free_lp_columns(sv._h, _iptr(FREE_LP), 1, 0.0)),
    "correctors": ("ipm_set_centrality_correctors", lambda sv: sv._lib.ipm_set_centrality_correctors(sv._h, 2)),
    "refinement": ("ipm_set_refinement", lambda sv: sv._lib.ipm_set_refinement(sv._h, 1)),
    "mehrotra_start": ("ipm_init_state_mehrotra", lambda sv: sv._lib.ipm_init_state_mehrotra(sv._h, None)),
}
# what a handle holds, by getter
HELD = {
    "quad": lambda sv: sv.quadratic_nonzeros() > 0, "free": lambda sv: sv.free_columns().shape[0] > 0, "free_lp": lambda sv: sv.free_lp_columns()[0].shape[0] > 0,
    "correctors": lambda sv: sv.corrector_info()["k"] > 0,
    "refinement": lambda sv: sv.refine_info().k > 0, "small_path": lambda sv: sv.schedule()["fused_small"] == 1, "mehrotra_start": lambda sv: False,
}
# the keywords of a handle that holds a feature (the partner b of a row, or its lift) on the 3 x 6 LP
HOLD = {
    "quad": dict(quad=G), "free": dict(quad=G, free=FREE), "free_lp": dict(free_lp=FREE_LP), "detect": dict(detect_infeasibility=True),
    "correctors": dict(correctors=2), "lockstep": dict(lockstep=True), "small_path": dict(sparse=True),
    "detect_qp": dict(detect_qp=True, quad=G), "small_quadratic_flag": dict(quad_small=True), "small_free_flag": dict(free_small=True),
}
# excluded pairs served elsewhere, each with its reason
DELEGATED = {
    ("lockstep", "bounds"): "joining a batch needs a lockstep-eligible handle of more than 128 rows: tests/test_gpu_lockstep_bounds.py",
    ("dense_split", "lockstep"): "ipm_set_dense_columns needs a sparse-factor handle of more than 128 rows: tests/test_gpu_dense_split.py",
}
FIXED_AT_CREATE = ("lockstep", "detect", "detect_qp")


def make(**kw):
    A = sparse.csc_matrix(A_) if kw.pop("sparse", False) else A_
    return ipm.IpmSolver(A, B_, C_, ub=UB, **kw)


def converges(sv):
    sv.init_state(1.0)
    st = sv.solve(tol=1e-8, max_iter=200)
    assert st["status"] == 1, st


EXCLUDED = [(a, b) for a, b in itertools.product(FEATURES, repeat=2) if compat(a, b)[0]]          # (host only: no device is touched)


def test_every_excluded_pair_has_a_recipe():
    assert len(EXCLUDED) >= 30
    for a, b in EXCLUDED:
        assert (a, b) in DELEGATED or a in FIXED_AT_CREATE or a == "small_path" or (a in SWITCH and b in HOLD), (a, b)
    for a, b in DELEGATED:
        assert compat(a, b)[0], (a, b)


@pytest.mark.parametrize("a,b", [p for p in EXCLUDED if p[0] in SWITCH and p not in DELEGATED], ids=lambda v: v)
def test_switching_on_beside_the_partner_is_refused(a, b):
    who, switch = SWITCH[a]
    lift = compat(a, b)[1]
    with make(**HOLD[b]) as sv:
        held = {f: HELD[f](sv) for f in HELD}
        assert held.get(b, True)
        rc = switch(sv)
        msg = sv._lib.ipm_last_error(sv._h).decode()
        assert rc == ERR_INVALID_ARG and msg.startswith(who + ": "), (rc, msg)
        assert {f: HELD[f](sv) for f in HELD} == held, msg                      # the handle keeps what it held
        converges(sv)                                                           # ... and stays usable
    if lift:                                                                    # the lifting flag: accepted
        kw = dict(HOLD[b], **HOLD[lift])
        if lift == "small_free_flag":
            kw.update(quad=G)                                                   # (a free column needs its term; IPM_FLAG_SMALL_FREE implies the quadratic flag)
        with make(**kw) as sv:
            if a == "quad":
                sv.set_quadratic(None)                                          # (detect_qp needs a term at construction: cleared, then set again)
                assert not HELD["quad"](sv)
            rc = switch(sv)
            assert rc == 0, sv._lib.ipm_last_error(sv._h)
            assert HELD[a](sv) and HELD.get(b, lambda s: True)(sv)
            converges(sv)


@pytest.mark.parametrize("b", [b for a, b in EXCLUDED if a == "small_path"])
def test_the_small_path_is_declined_not_refused(b):
    """ipm_set_A_csc beside a feature the one-workgroup kernel lacks: the multi-kernel path, no error; with the lifting flag the small path."""
    lift = compat("small_path", b)[1]
    with make(sparse=True, **HOLD[b]) as sv:
        assert not HELD["small_path"](sv) and HELD[b](sv)
        converges(sv)
    with make(sparse=True) as sv:                                               # (the LP alone does take the path)
        assert HELD["small_path"](sv)
    if lift:
        with make(sparse=True, **dict(HOLD[b], **HOLD[lift])) as sv:
            assert HELD["small_path"](sv) and HELD[b](sv)
            converges(sv)


def test_flags_that_exclude_each_other_are_refused_by_ipm_create():
    assert compat("detect_qp", "lockstep") == (True, None) and compat("lockstep", "detect_qp") == (True, None)
    lib = ipm.load_library()
    opts = _lib.Options()
    lib.ipm_default_options(C.byref(opts))
    opts.flags = _lib.FLAG_LOCKSTEP | _lib.FLAG_DETECT_INFEASIBILITY | _lib.FLAG_DETECT_QUADRATIC
    h = C.c_void_p()
    assert lib.ipm_create(0, 3, 6, C.byref(opts), None, 0, None, C.byref(h)) == ERR_INVALID_ARG and not h.value
    assert lib.ipm_last_error(None).decode().startswith("ipm_create: IPM_FLAG_DETECT_QUADRATIC with IPM_FLAG_LOCKSTEP (")
