"""interiorpointmethod_amd -- MI355X-native Newton/KKT hot path of a Mehrotra interior-point
LP solver (drop-in for the loop of payakorn/InteriorPointMethod)."""
from .analysis import dense_columns  # noqa: F401
from ._lib import IpmError, IpmLibraryError, LIB_PATH, load as load_library  # noqa: F401
from .general_form import add_bound_into_matrix, get_Abc, new_interior_sparse  # noqa: F401
from .solver import (IpmSolver, LockstepBatch, direction_corrected, direction_corrected_sparse, direction_predicted,  # noqa: F401
                     direction_predicted_sparse,
                     init_small_batch_mehrotra, interior, interior_sparse, last_info, lockstep_eligible, lu_factor, lu_solve, small_batch_eligible, solve, solve_linear,
                     solve_lockstep, solve_small_batch, solve_small_batch_solvers, solve_small_qp_batch, solve_with_info, verify_certificate,
                     factor_qp_form, solve_factor_qp, solve_small_factor_qp_batch, solve_small_qp_batch_detect, solve_small_factor_qp_batch_detect)

__all__ = ["IpmSolver", "solve", "solve_with_info", "interior", "interior_sparse",
           "direction_predicted_sparse", "direction_corrected_sparse", "direction_predicted", "direction_corrected", "solve_linear", "lu_solve", "lu_factor", "last_info",
           "solve_lockstep", "LockstepBatch", "solve_small_batch", "solve_small_batch_solvers", "solve_small_qp_batch", "factor_qp_form", "solve_factor_qp", "solve_small_factor_qp_batch", "init_small_batch_mehrotra", "small_batch_eligible", "verify_certificate", "lockstep_eligible", "new_interior_sparse", "get_Abc", "add_bound_into_matrix", "dense_columns",
           "solve_small_qp_batch_detect", "solve_small_factor_qp_batch_detect",
           "IpmError", "IpmLibraryError", "load_library", "LIB_PATH"]
