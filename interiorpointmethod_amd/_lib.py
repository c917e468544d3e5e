"""ctypes binding of libipm_hip.so (C ABI declared in include/ipm_hip.h).

The HIP library IS the product path: there is no CPU fallback.  ``load()`` raises
``IpmLibraryError`` when the shared object has not been built (run
``python -c "import __graft_entry__ as g; g.build()"``) and every compute entry
point raises ``IpmError`` with the library's message on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libipm_hip.so")

# symbols declared in include/ipm_hip.h (checked by tests/test_abi.py against the header)
EXPORTS = [
    "ipm_abi_version", "ipm_device_count", "ipm_default_options", "ipm_workspace_bytes", "ipm_workspace_bytes_csc", "ipm_workspace_bytes_opts",
    "ipm_create", "ipm_destroy", "ipm_last_error", "ipm_set_A_dense", "ipm_set_A_csc",
    "ipm_set_bc", "ipm_set_state", "ipm_get_state", "ipm_init_state", "ipm_init_state_mehrotra", "ipm_set_bounds", "ipm_set_bound_state", "ipm_get_bound_state", "ipm_set_quadratic", "ipm_get_quadratic", "ipm_set_free_columns", "ipm_get_free_columns", "ipm_set_free_lp_columns", "ipm_get_free_lp_columns", "ipm_debug_get_column_vector", "ipm_equilibrate", "ipm_get_scaling", "ipm_newton_direction",
    "ipm_iterate", "ipm_solve", "ipm_solve_batch", "ipm_solve_small_batch", "ipm_init_small_batch_mehrotra", "ipm_batch_create", "ipm_batch_destroy", "ipm_batch_last_error", "ipm_batch_add", "ipm_batch_step", "ipm_batch_stats", "ipm_get_history", "ipm_set_centrality_correctors", "ipm_get_corrector_info", "ipm_set_refinement", "ipm_get_refinement_info", "ipm_debug_get_refine_vector", "ipm_set_infeasibility_tol", "ipm_get_certificate", "ipm_get_schedule", "ipm_get_schedule_words", "ipm_debug_at_pieces", "ipm_debug_chol_plan", "ipm_debug_step_kernel", "ipm_debug_step_kernel_ex", "ipm_debug_compat", "ipm_order_rows", "ipm_get_factor_info", "ipm_solve_linear", "ipm_lu_solve", "ipm_lu_factor", "ipm_normal_solve", "ipm_form_normal_matrix", "ipm_get_factor",
    "ipm_set_dense_columns", "ipm_get_dense_split_info", "ipm_debug_get_dense_split",
    "ipm_set_profiling", "ipm_get_phase_ms", "ipm_debug_get_stamps", "ipm_debug_ff_schedule", "ipm_debug_ff_trace", "ipm_debug_get_block_inverse", "ipm_debug_get_group_inverse", "ipm_debug_ls_merge",
    "ipm_debug_batch_schedule",
    "ipm_debug_guard_list", "ipm_debug_guard_check", "ipm_debug_guard_log", "ipm_debug_guard_layout", "ipm_debug_guard_compare",
]

IPM_OK = 0
STATUS_RUNNING, STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_NAN = 0, 1, 2, 3
STATUS_PRIMAL_INFEASIBLE, STATUS_DUAL_INFEASIBLE = 5, 6     # with FLAG_DETECT_INFEASIBILITY only
FLAG_NO_DEVICE_POLLING = 1      # include/ipm_hip.h: IPM_FLAG_NO_DEVICE_POLLING
FLAG_NO_AUTO_REGULARIZE = 2     # include/ipm_hip.h: IPM_FLAG_NO_AUTO_REGULARIZE
FLAG_SINGLE_STREAM = 4          # include/ipm_hip.h: IPM_FLAG_SINGLE_STREAM
FLAG_SPARSE_FACTOR = 8          # include/ipm_hip.h: IPM_FLAG_SPARSE_FACTOR
FLAG_LOCKSTEP = 16              # include/ipm_hip.h: IPM_FLAG_LOCKSTEP
FLAG_DETECT_INFEASIBILITY = 32  # include/ipm_hip.h: IPM_FLAG_DETECT_INFEASIBILITY
FLAG_SMALL_QUADRATIC = 64       # include/ipm_hip.h: IPM_FLAG_SMALL_QUADRATIC
FLAG_LOCKSTEP_BOUNDS = 128      # include/ipm_hip.h: IPM_FLAG_LOCKSTEP_BOUNDS
# Flags the header states by a shift expression after IPM_FLAG_LOCKSTEP_BOUNDS.  They are attributes of this module like the ones
# above (_lib.FLAG_SMALL_FREE; module __getattr__ below) but not names of its dict: tests/test_lockstep_bounds_host.py pins the set
# of FLAG_* names the dict holds.
_SHIFTED_FLAGS = {"FLAG_SMALL_FREE": FLAG_LOCKSTEP_BOUNDS << 1,          # include/ipm_hip.h: IPM_FLAG_SMALL_FREE (256)
                  "FLAG_DETECT_QUADRATIC": FLAG_LOCKSTEP_BOUNDS << 2}    # include/ipm_hip.h: IPM_FLAG_DETECT_QUADRATIC (512)


def __getattr__(name):
    if name in _SHIFTED_FLAGS:
        return _SHIFTED_FLAGS[name]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


ERR_WORKSPACE = -4
ABI_VERSION = 4
HISTORY_CAPACITY = 1024         # IPM_HISTORY_CAPACITY
MAX_CORRECTORS = 8              # include/ipm_hip.h: IPM_MAX_CORRECTORS
MAX_REFINE = 4                  # include/ipm_hip.h: IPM_MAX_REFINE
MAX_DENSE_COLS = 64             # include/ipm_hip.h: IPM_MAX_DENSE_COLS
FREE_LP_RHO_DEFAULT = 1e-8      # include/ipm_hip.h: IPM_FREE_LP_RHO_DEFAULT
# include/ipm_hip.h: IPM_FEATURE_*, by id (ipm_debug_compat; the `pair` of a row of options.ROWS names two of them)
FEATURES = ("bounds", "quad", "free", "free_lp", "detect", "detect_qp", "correctors", "refinement", "dense_split", "lockstep", "lockstep_bounds",
            "small_path", "mehrotra_start", "small_quadratic_flag", "small_free_flag")
ERR_INVALID_INPUT = -6
ERR_SINGULAR = -7               # include/ipm_hip.h: IPM_ERR_SINGULAR (ipm_lu_solve / ipm_lu_factor, info > 0)


class IpmLibraryError(RuntimeError):
    """libipm_hip.so is missing or does not export the ABI."""


class IpmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libipm_hip status %d: %s" % (code, msg))
        self.code = code


class Options(C.Structure):
    _fields_ = [("eta", C.c_double), ("pivot_guard_eps", C.c_double), ("pivot_guard_big", C.c_double),
                ("check_every", C.c_int32), ("flags", C.c_int32), ("sparse_nnz", C.c_int64),
                ("regularize", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("pivots_fixed", C.c_int32),
                ("auto_regularized", C.c_int32), ("objective", C.c_double), ("rp_norm", C.c_double),
                ("rd_norm", C.c_double), ("gap", C.c_double), ("b_norm", C.c_double),
                ("c_norm", C.c_double), ("mu", C.c_double), ("mu_aff", C.c_double),
                ("sigma", C.c_double), ("alpha_aff_p", C.c_double), ("alpha_aff_d", C.c_double),
                ("alpha_p", C.c_double), ("alpha_d", C.c_double), ("solve_ms", C.c_double),
                ("objective_last_finite", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IterRecord(C.Structure):
    """ipm_iter_record: one per completed iteration (the line the reference prints, main.py:808-809, :1186)."""
    _fields_ = [("k", C.c_int32), ("pivots_fixed", C.c_int32), ("objective", C.c_double), ("rp_norm", C.c_double),
                ("rd_norm", C.c_double), ("gap", C.c_double), ("mu", C.c_double), ("sigma", C.c_double),
                ("alpha_aff_p", C.c_double), ("alpha_aff_d", C.c_double), ("alpha_p", C.c_double),
                ("alpha_d", C.c_double)]


class GuardBand(C.Structure):
    """ipm_guard_band: one guard band of the test knob IPM_TEST_ALLOC_GUARD (include/ipm_hip.h)."""
    _fields_ = [("tag", C.c_char * 96), ("address", C.c_uint64), ("bytes", C.c_uint64), ("inner", C.c_uint64), ("inner_bytes", C.c_uint64),
                ("side", C.c_int32), ("device", C.c_int32), ("byte", C.c_int32), ("ordinal", C.c_int32), ("first_bad", C.c_int64),
                ("bad_count", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["tag"] = self.tag.decode()
        return d


_lib = None


def load():
    """Load the shared library once; fail loudly when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64/libhsa-runtime64 and preloads them by path.  Two HSA
    # runtimes cannot share one process (the second sees no device), so when torch is
    # installed it is imported FIRST: libipm_hip.so's NEEDED libamdhip64.so.7 then resolves to
    # the copy torch already mapped.  Without torch the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover
        pass
    if not os.path.exists(LIB_PATH):
        raise IpmLibraryError(
            "%s not found: the HIP extension has not been built. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback." % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise IpmLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise IpmLibraryError("%s lacks symbols %s" % (LIB_PATH, missing))
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pd = C.POINTER(C.c_double)
    lib.ipm_abi_version.restype = C.c_int
    lib.ipm_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.ipm_default_options.argtypes = [C.POINTER(Options)]
    lib.ipm_default_options.restype = None
    lib.ipm_workspace_bytes.argtypes = [i64, i64, C.POINTER(C.c_size_t)]
    lib.ipm_workspace_bytes_csc.argtypes = [i64, i64, i64, C.POINTER(C.c_size_t)]
    lib.ipm_workspace_bytes_opts.argtypes = [i64, i64, C.POINTER(Options), C.POINTER(C.c_size_t)]
    lib.ipm_create.argtypes = [C.c_int, i64, i64, C.POINTER(Options), vp, C.c_size_t, vp, C.POINTER(vp)]
    lib.ipm_destroy.argtypes = [vp]
    lib.ipm_last_error.argtypes = [vp]
    lib.ipm_last_error.restype = C.c_char_p
    lib.ipm_set_A_dense.argtypes = [vp, vp, i64, C.c_int]
    lib.ipm_set_A_csc.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), pd, i64]
    lib.ipm_set_bc.argtypes = [vp, pd, pd]
    lib.ipm_set_state.argtypes = [vp, pd, pd, pd]
    lib.ipm_get_state.argtypes = [vp, pd, pd, pd]
    lib.ipm_init_state.argtypes = [vp, dbl]
    lib.ipm_init_state_mehrotra.argtypes = [vp, C.POINTER(i32)]
    lib.ipm_set_bounds.argtypes = [vp, pd]
    lib.ipm_set_bound_state.argtypes = [vp, pd, pd]
    lib.ipm_get_bound_state.argtypes = [vp, pd, pd]
    lib.ipm_set_quadratic.argtypes = [vp, pd]
    lib.ipm_get_quadratic.argtypes = [vp, pd, C.POINTER(i64)]
    lib.ipm_set_free_columns.argtypes = [vp, C.POINTER(i32), i32]
    lib.ipm_get_free_columns.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.ipm_set_free_lp_columns.argtypes = [vp, C.POINTER(i32), i32, dbl]
    lib.ipm_get_free_lp_columns.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32), pd]
    lib.ipm_debug_get_column_vector.argtypes = [vp, i32, pd]
    lib.ipm_equilibrate.argtypes = [vp, i32, pd]
    lib.ipm_get_scaling.argtypes = [vp, pd, pd]
    lib.ipm_newton_direction.argtypes = [vp, C.c_int, pd, pd, pd, C.POINTER(Stats)]
    lib.ipm_iterate.argtypes = [vp, i32, C.POINTER(Stats)]
    lib.ipm_solve.argtypes = [vp, dbl, dbl, dbl, i32, C.POINTER(Stats)]
    lib.ipm_solve_batch.argtypes = [C.POINTER(vp), i32, dbl, dbl, dbl, i32, C.POINTER(Stats)]
    lib.ipm_solve_small_batch.argtypes = [C.POINTER(vp), i32, dbl, dbl, dbl, i32, vp, C.POINTER(Stats)]
    lib.ipm_init_small_batch_mehrotra.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(i32)]
    lib.ipm_batch_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.ipm_batch_destroy.argtypes = [vp]
    lib.ipm_batch_last_error.argtypes = [vp]
    lib.ipm_batch_last_error.restype = C.c_char_p
    lib.ipm_batch_add.argtypes = [vp, vp, dbl, dbl, dbl, i32, C.POINTER(i32)]
    lib.ipm_batch_step.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32), C.POINTER(i32)]
    lib.ipm_batch_stats.argtypes = [vp, i32, C.POINTER(Stats)]
    lib.ipm_get_history.argtypes = [vp, C.POINTER(IterRecord), i32, C.POINTER(i32)]
    lib.ipm_set_centrality_correctors.argtypes = [vp, i32]
    lib.ipm_get_corrector_info.argtypes = [vp, C.POINTER(i64)]
    lib.ipm_set_refinement.argtypes = [vp, i32]
    lib.ipm_get_refinement_info.argtypes = [vp, pd]
    lib.ipm_debug_get_refine_vector.argtypes = [vp, i32, pd, i64, C.POINTER(i64)]
    lib.ipm_get_schedule.argtypes = [vp, C.POINTER(i32)]
    lib.ipm_get_schedule_words.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.ipm_debug_at_pieces.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(i32)]
    lib.ipm_debug_chol_plan.argtypes = [i32, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32]
    lib.ipm_debug_step_kernel.argtypes = [i32, i32, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]
    lib.ipm_debug_step_kernel_ex.argtypes = [i32, i32, i32, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]
    lib.ipm_debug_compat.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)]
    pg, u64 = C.POINTER(GuardBand), C.c_uint64
    lib.ipm_debug_guard_list.argtypes = [vp, pg, i32, C.POINTER(i32)]
    lib.ipm_debug_guard_check.argtypes = [vp, pg, i32, C.POINTER(i32)]
    lib.ipm_debug_guard_log.argtypes = [pg, i32, C.POINTER(i32)]
    lib.ipm_debug_guard_layout.argtypes = [i64, i64, C.POINTER(Options), pg, i32, C.POINTER(i32), C.POINTER(u64), C.POINTER(u64)]
    lib.ipm_debug_guard_compare.argtypes = [C.c_char_p, u64, i32, C.POINTER(i64), C.POINTER(i64)]
    lib.ipm_set_infeasibility_tol.argtypes = [vp, dbl, dbl]
    lib.ipm_get_certificate.argtypes = [vp, pd, pd, pd, pd]
    lib.ipm_order_rows.argtypes = [i64, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), pd]
    lib.ipm_get_factor_info.argtypes = [vp, C.POINTER(i64)]
    lib.ipm_solve_linear.argtypes = [vp, pd, i64, pd, pd, C.POINTER(i32)]
    lib.ipm_lu_solve.argtypes = [C.c_int, i64, pd, i64, i64, pd, i64, pd, i64, C.POINTER(i64)]
    lib.ipm_lu_factor.argtypes = [C.c_int, i64, pd, i64, pd, i64, C.POINTER(i32), C.POINTER(i64)]
    lib.ipm_normal_solve.argtypes = [vp, pd, pd, pd, C.c_int, C.POINTER(i32)]
    lib.ipm_form_normal_matrix.argtypes = [vp, pd, pd, i64]
    lib.ipm_get_factor.argtypes = [vp, pd, i64]
    lib.ipm_set_dense_columns.argtypes = [vp, i32, C.POINTER(i32)]
    lib.ipm_get_dense_split_info.argtypes = [vp, C.POINTER(i64)]
    lib.ipm_debug_get_dense_split.argtypes = [vp, i32, pd, i64, C.POINTER(i64)]
    lib.ipm_set_profiling.argtypes = [vp, C.c_int]
    lib.ipm_get_phase_ms.argtypes = [vp, pd]
    lib.ipm_debug_get_stamps.argtypes = [vp, C.POINTER(C.c_longlong)]
    lib.ipm_debug_ff_schedule.argtypes = [i32, i32, i32, C.POINTER(C.c_ubyte), i32, C.POINTER(i32), C.POINTER(i32), pd]
    lib.ipm_debug_get_block_inverse.argtypes = [vp, i32, pd]
    lib.ipm_debug_get_group_inverse.argtypes = [vp, i32, i32, pd]
    lib.ipm_debug_ff_trace.argtypes = [vp, C.POINTER(C.c_longlong), i64, C.POINTER(i64), C.POINTER(C.c_ubyte), C.POINTER(i32)]
    lib.ipm_debug_ls_merge.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), i32, i32, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.ipm_debug_batch_schedule.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(i32)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("ipm_default_options", "ipm_last_error", "ipm_batch_last_error"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def check(handle, code):
    if code != IPM_OK:
        msg = load().ipm_last_error(handle)
        raise IpmError(code, (msg or b"").decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    load().ipm_device_count(C.byref(n))
    return n.value



# ---- the guard bands of the test knob IPM_TEST_ALLOC_GUARD (include/ipm_hip.h: ipm_debug_guard_*), as lists of dicts
def _guard_records(call, capacity=4096):
    out, count = (GuardBand * capacity)(), C.c_int32(0)
    check(None, call(out, capacity, C.byref(count)))
    if count.value > capacity:
        return _guard_records(call, count.value)
    return [out[i].as_dict() for i in range(count.value)]


def guard_list(handle=None):
    """The live bands of a handle (its C pointer), or of the process."""
    return _guard_records(lambda out, cap, cnt: load().ipm_debug_guard_list(handle, out, cap, cnt))


def guard_check(handle=None):
    """The DAMAGED bands among them, compared now (synchronises the device)."""
    return _guard_records(lambda out, cap, cnt: load().ipm_debug_guard_check(handle, out, cap, cnt))


def guard_log():
    """Reads and clears the log of the damage found when guarded memory was released."""
    return _guard_records(lambda out, cap, cnt: load().ipm_debug_guard_log(out, cap, cnt))
