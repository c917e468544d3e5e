"""The host side above the C ABI under its historical name: every name is re-exported from the module that owns it.

    analysis.py   host analysis of an LP: row orders, the factor="auto" model, flop counts, prepare()
    handle.py     IpmSolver, the handle class
    batches.py    the lockstep batch and the small-LP batch
    api.py        solve, solve_with_info, interior*, verify_certificate: the reference's call surface
    factor_qp.py  factor_qp_form, solve_factor_qp, solve_small_factor_qp_batch: diagonal-plus-low-rank QPs on the free-column iteration
    kkt.py        direction_*, solve_linear, the unreduced KKT system and the device LU
(to replace a name for a test, patch it on the owning module: a function looks its collaborators up there)"""
from .analysis import (FUSED_SMALL_MAX_ROWS, REORDER_MIN_ROWS, SPARSE_FACTOR_MIN_ROWS, Prepared, _col, _tile_envelope_work,  # noqa: F401
                       _upper_bounds, _worth_ordering, dense_tile_ms, envelope_row_order, factor_flops, path_flops, prefer_sparse_factor,
                       prepare, sparse_factor_order)
from .handle import SCALE_PASSES, STATUS_NAMES, IpmSolver, _dptr, check_free, check_free_lp, check_free_rho, check_scale, mehrotra_started, shift_allowed, wants_shift  # noqa: F401
from .api import _info, _verdict, interior, interior_sparse, last_info, solve, solve_with_info, unscaled_residuals, verify_certificate  # noqa: F401
from .batches import (LockstepBatch, _small_batch_host_check, _small_qp_batch_host_check, init_small_batch_mehrotra, lockstep_eligible,  # noqa: F401
                      small_batch_eligible, solve_lockstep, solve_small_batch, solve_small_batch_solvers, solve_small_qp_batch, solve_small_qp_batch_detect)
from .factor_qp import _small_factor_qp_host_check, factor_qp_form, factor_qp_solution, solve_factor_qp, solve_small_factor_qp_batch, solve_small_factor_qp_batch_detect  # noqa: F401
from .kkt import (_METHODS, _dense, _kkt_corrected, _kkt_matrix, _kkt_predicted, _kkt_residuals, _kkt_solve, _lu_error, _ratio,  # noqa: F401
                  _square, direction_corrected, direction_corrected_sparse, direction_predicted, direction_predicted_sparse,
                  lu_factor, lu_solve, solve_linear)
