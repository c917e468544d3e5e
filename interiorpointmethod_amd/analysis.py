"""Host analysis of one LP (no device is touched): row orders, the factor="auto" model, bench.py's flop counts, `prepare`."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .options import refuse_dense_cols          # noqa: F401  (its importers find it here as before)

try:  # scipy is optional on the host side (dense inputs work without it)
    from scipy import sparse as _sp
except Exception:  # pragma: no cover
    _sp = None

REORDER_MIN_ROWS = 2048      # below this the factorization is a latency chain; reordering buys nothing
SPARSE_FACTOR_MIN_ROWS = 600          # below five 128-row blocks the dense chain is shorter than one tree sweep set
FUSED_SMALL_MAX_ROWS = 128            # sparse handles up to this many rows run the fused single-workgroup kernel (small_lp.h)


def _is_sparse(A):
    return _sp is not None and _sp.issparse(A)


def _tile_envelope_heights(P, nb=128):
    """Envelope height, in blocks below the diagonal block, of every nb-column block of the symmetric pattern P."""
    P = P.tocoo()
    nblk = (P.shape[0] + nb - 1) // nb
    last = np.arange(nblk)
    np.maximum.at(last, np.minimum(P.row, P.col) // nb, np.maximum(P.row, P.col) // nb)
    return np.maximum.accumulate(last) - np.arange(nblk)


def _tile_envelope_work(P, nb=128):
    """Sum over 128-column blocks of (envelope height in blocks)^2 for the symmetric pattern P: the work measure the
    blocked Cholesky in libipm_hip pays (it skips the blocks below the tile envelope) -> (that sum, the same for a dense P)."""
    hgt = _tile_envelope_heights(P, nb)
    return float(np.sum(hgt ** 2)), float(np.sum((hgt.shape[0] - 1 - np.arange(hgt.shape[0])) ** 2))


def envelope_row_order(A, force=False):
    """Reverse Cuthill-McKee order of the rows of A on the pattern of A A^T, or None when it does not shrink the
    tile envelope of the normal matrix by at least 30 % (force=True: always the RCM order).  The row order of A is the caller's to choose: y and dy are
    permuted back, x and s are untouched, so the solver seam is unchanged (the reference's SuperLU also reorders
    internally, COLAMD, main.py:180)."""
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    P = abs(A) @ abs(A).T
    P = _sp.csr_matrix(P)
    P.data[:] = 1.0
    perm = np.asarray(reverse_cuthill_mckee(P, symmetric_mode=True), dtype=np.int64)
    before, dense = _tile_envelope_work(P)
    after, _ = _tile_envelope_work(P[perm][:, perm])
    if force or after < 0.7 * min(before, dense):
        return perm
    return None


def sparse_factor_order(A, alternative_ms=0.0):
    """Fill-reducing row order for the multifrontal sparse Cholesky (ipm_order_rows: minimum degree + elimination-tree
    postorder, host only) -> (perm, info) with info = dict(nnz_pattern, nnz_factor, flops, height), or (None, None)
    when A A^T is too dense for it.  The reference gets this from SuperLU's COLAMD inside spsolve (main.py:180).
    alternative_ms > 0: the predicted ms per iteration of the dense-tile path; the elimination then gives up (None, None)
    at the first pivot whose degree shows that the sparse factor cannot beat it (factor="auto" passes it, "sparse" does not)."""
    lib = _lib.load()
    A = _sp.csc_matrix(A)
    m, n = A.shape
    perm = np.zeros(m, dtype=np.int32)
    info = np.zeros(8)
    if alternative_ms > 0.0:
        info[0], info[1] = float(alternative_ms), -1.0     # (marker: include/ipm_hip.h)
    ip = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ii = np.ascontiguousarray(A.indices, dtype=np.int32)
    rc = lib.ipm_order_rows(m, n, ip.ctypes.data_as(C.POINTER(C.c_int32)), ii.ctypes.data_as(C.POINTER(C.c_int32)),
                            perm.ctypes.data_as(C.POINTER(C.c_int32)), info.ctypes.data_as(C.POINTER(C.c_double)))
    if rc == _lib.ERR_WORKSPACE:
        return None, None
    _lib.check(None, rc)
    return perm.astype(np.int64), dict(nnz_pattern=int(info[0]), nnz_factor=int(info[1]), flops=float(info[2]),
                                       height=int(info[3]), panel_height=int(info[4]), path_area=float(info[5]),
                                       panels=int(info[6]), widest_front=int(info[7]))


def prefer_sparse_factor(m, info, dense_blocks):
    """The rule of factor="auto", fitted to measurements on MI355X (tools/sparse_factor_check.py, one LP on the GPU, ms per
    iteration sparse / dense): STOCFOR3 1.16 / 14.0, SIERRA 0.64 / 2.2, STOCFOR2 0.49 / 1.47, CZPROB 0.60 / 0.92, SCTAP3
    0.57 / 0.92, SHELL 0.48 / 0.67, GFRD-PNC 0.36 / 0.65, SCTAP2 0.66 / 0.84, 80BAU3B 2.6 / 3.35, GANGES 1.01 / 1.13 -- but
    25FV47 1.34 / 0.70, NESM 2.85 / 1.77, GREENBEA 3.2 / 1.73, BNL2 4.4 / 1.62, D2Q06C 6.4 / 1.56, PILOTNOV 3.3 / 0.91, GROW15
    2.66 / 0.71.  The sparse factor walks the panel tree five times per iteration and every level is a hand-off between
    workgroups: 0.061 ms per level of the panel tree plus 3.5e-6 ms per (front rows)^2 along the critical path (round 2: least
    squares over 23 LPs gave 5.6e-6, worst error 0.3 ms; round 3: the update of the large fronts moved to the matrix cores and
    13 re-measured LPs give 2.6e-6 .. 5.3e-6, BNL2 4.4 -> 2.8, D2Q06C 6.4 -> 4.15, PILOTNOV 3.3 -> 2.3, 25FV47 1.34 -> 0.99 ms; info["panel_height"], info["path_area"] from ipm_order_rows).  The dense-tile
    path walks a chain of m/128 pivot blocks at 0.08 ms each and does its flops on the matrix cores.  A predicted gain of
    10 % switches paths: of the 23 measured LPs only SCFXM3 (0.54 / 0.63, predicted 0.86) is on the slower path."""
    if info is None or m < SPARSE_FACTOR_MIN_ROWS or info.get("panel_height", 0) <= 0:
        return False
    t_sparse = max(0.3, -0.13 + 0.061 * info["panel_height"] + 3.5e-6 * info["path_area"])      # ms per iteration
    return 1.1 * t_sparse < dense_tile_ms(dense_blocks)


def dense_tile_ms(dense_blocks):
    """Predicted ms per iteration of the dense-tile path (0.1 + 0.08 per 128-row block, fitted with the rule above)."""
    return 0.1 + 0.08 * dense_blocks


def _worth_ordering(A):
    """Cheap screen before the minimum-degree ordering: an upper bound on the entries of A A^T (sum over columns of
    c (c - 1) / 2).  Beyond a few million the factor is close to dense and the ordering would only burn host time."""
    c = np.diff(A.indptr).astype(np.float64)
    return float(np.sum(c * (c - 1.0) / 2.0)) <= 4.0e6


def _factor_arg(factor):           # the argument, else the environment's IPM_FACTOR (read per call), else "auto"
    return factor or os.environ.get("IPM_FACTOR", "auto")


def _factor_path(A, m, factor):
    """THE rule of the factorization path of one LP (A: canonical CSC or an ndarray) -> (path, perm, info): "sparse" with the
    minimum-degree row order and the ipm_order_rows record, or "dense" with (None, None) (the envelope order is prepare's next step).
    An LP of at most FUSED_SMALL_MAX_ROWS rows runs the fused single-workgroup kernel, which builds no sparse factor: its path is
    "dense" whatever is asked, and "auto" does not order it.  factor="sparse" on such an LP keeps the minimum-degree order all the
    same: the fused kernel has always run on A in that row order, and y is bit-identical only in the same order."""
    dense = ("dense", None, None)
    if not _is_sparse(A) or factor == "dense":
        return dense
    forced, small, blocks = factor == "sparse", m <= FUSED_SMALL_MAX_ROWS, (m + 127) // 128
    if not forced and (small or m < SPARSE_FACTOR_MIN_ROWS or not _worth_ordering(A)):
        return dense
    perm, info = sparse_factor_order(A, 0.0 if forced else dense_tile_ms(blocks))
    if perm is None:
        return dense
    if small:
        return "dense", perm, None
    if forced or prefer_sparse_factor(m, info, blocks):
        return "sparse", perm, info
    return dense


# THE selection rule of the dense-column split, stated once: a column is dense when it has more than
# max(DENSE_COL_FRAC * m, DENSE_COL_FLOOR) entries.  Fixed by a host survey of the standard-form Netlib fixtures (tests/golden): with
# 0.1 and 30 the rule takes 22 columns of FIT1P (m = 1026; nnz(A A^T) / m^2 0.37 -> 0.017 without them), 14 of SEBA (1029; 0.10 ->
# 0.003) and 22 of ISRAEL (174; 0.74 -> 0.12), leaves no row of the three empty, and takes nothing from the files whose A A^T is
# sparse already.  The floor keeps a small LP (0.1 m below 30) from calling its ordinary columns dense.
DENSE_COL_FRAC = 0.1
DENSE_COL_FLOOR = 30
MAX_DENSE_COLS = _lib.MAX_DENSE_COLS


def dense_columns(A, max_cols=MAX_DENSE_COLS, frac=DENSE_COL_FRAC, floor=DENSE_COL_FLOOR):
    """The columns of sparse A to split out of the sparse factor (IpmSolver(dense_cols=...)) -> ascending int32 indices: those
    with more than max(frac * m, floor) entries, the densest first (ties: the lower index) up to max_cols <= MAX_DENSE_COLS, and
    never one whose removal, with the ones already taken, would leave a row of A without an entry.  Host only."""
    if not 0 <= int(max_cols) <= MAX_DENSE_COLS:
        raise ValueError("max_cols must be 0 .. %d, not %r" % (MAX_DENSE_COLS, max_cols))
    if not _is_sparse(A):
        return np.zeros(0, dtype=np.int32)
    A = _sp.csc_matrix(A)
    m = A.shape[0]
    cnt = np.diff(A.indptr)
    cand = np.flatnonzero(cnt > max(frac * m, floor))
    cand = cand[np.lexsort((cand, -cnt[cand]))]
    left = np.bincount(A.indices, minlength=m)          # entries a row keeps
    out = []
    for j in cand:
        if len(out) >= int(max_cols):
            break
        rows = A.indices[A.indptr[j]:A.indptr[j + 1]]
        if (left[rows] <= 1).any():
            continue
        left[rows] -= 1
        out.append(int(j))
    return np.asarray(sorted(out), dtype=np.int32)


def check_dense_cols(dense_cols, n):
    """THE host check of an explicit dense_cols sequence -> int32 array: distinct indices 0 .. n-1, at most MAX_DENSE_COLS."""
    cols = np.asarray(dense_cols).reshape(-1)
    if cols.size and not np.issubdtype(cols.dtype, np.integer):
        raise ValueError("dense_cols must be None, \"auto\" or a sequence of column indices")
    cols = cols.astype(np.int64)
    if cols.size > MAX_DENSE_COLS:
        raise ValueError("dense_cols: %d columns exceed the %d the split takes" % (cols.size, MAX_DENSE_COLS))
    if cols.size and (cols.min() < 0 or cols.max() >= n):
        raise ValueError("dense_cols: column index out of range 0 .. %d" % (n - 1))
    if np.unique(cols).size != cols.size:
        raise ValueError("dense_cols: duplicated column index")
    return cols.astype(np.int32)


def without_columns(A, cols):
    """Canonical CSC of A with the columns `cols` emptied (same shape): the matrix the sparse factor is built from under a split."""
    A = _sp.csc_matrix(A)
    keep = np.ones(A.shape[1], dtype=bool)
    keep[cols] = False
    cnt = np.diff(A.indptr)
    entry = np.repeat(keep, cnt)
    indptr = np.concatenate(([0], np.cumsum(np.where(keep, cnt, 0)))).astype(A.indptr.dtype)
    As = _sp.csc_matrix((A.data[entry], A.indices[entry], indptr), shape=A.shape)
    return As


def path_flops(A, factor=None, want_info=False):
    """(path, Cholesky flops, flops of the four triangular sweeps) of one iteration AS THE DEVICE RUNS IT for this A under
    IpmSolver's factor rule: the sparse factor costs sum over columns of (entries of the column)^2 and 4 nnz(L); the
    dense-tile path factor_flops(A) and 4 m^2.  bench.py's roofline denominator for the Netlib runs.
    want_info: a fourth value, the ipm_order_rows info of an LP put on the sparse factor (None otherwise)."""
    m = A.shape[0]
    path, _, info = _factor_path(_sp.csc_matrix(A) if _is_sparse(A) else A, m, _factor_arg(factor))
    if path == "sparse":
        out = ("sparse", float(info["flops"]), 4.0 * info["nnz_factor"])
    else:
        out = ("dense", factor_flops(A), 4.0 * m * m)
    return out + (info,) if want_info else out


def factor_flops(A, nb=128):
    """Flops of the blocked Cholesky of A A^T AS THE DEVICE RUNS IT for this A: dense handles and sparse handles whose
    tile envelope removes less than 20 % of the work factor the full matrix (m^3/3); otherwise only the blocks inside
    the tile envelope (after the reverse Cuthill-McKee row order where IpmSolver applies it) are touched:
    sum over block columns of nb^3 (h^2 + 2 h + 1/3), h = envelope height in blocks below the diagonal block.
    Used by bench.py for the roofline denominator of the Netlib runs -- STOCFOR3's factor is 11 % of m^3/3."""
    m = A.shape[0]
    if not _is_sparse(A):
        return m ** 3 / 3.0
    P = _sp.csr_matrix(abs(A) @ abs(A).T)
    P.data[:] = 1.0
    if m >= REORDER_MIN_ROWS:
        perm = envelope_row_order(A)
        if perm is not None:
            P = P[perm][:, perm]
    work, dense = _tile_envelope_work(P, nb)
    if not work < 0.8 * dense:                   # the library's rule (ipm_set_A_csc): the envelope must remove work
        return m ** 3 / 3.0
    hgt = _tile_envelope_heights(P, nb).astype(np.float64)
    return float(np.sum(nb ** 3 * (hgt * hgt + 2.0 * hgt + 1.0 / 3.0)))


def _col(v, n, name):
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if v.shape[0] != n:
        raise ValueError("%s has length %d, expected %d" % (name, v.shape[0], n))
    return v


class Prepared:
    """The host-side analysis of one LP -- what IpmSolver does before it touches the device: canonical A, the factorization
    path (factor="auto" rule), the fill-reducing or envelope row order and A, b in that order.  `prepare` builds it and
    IpmSolver(..., prepared=P) takes it.  (Computing it AHEAD of the solves on helper threads in the batched mode was tried and
    is slower -- 14.55 -> 13.2 LPs/s on the 73-LP suite: the helpers' SciPy sections hold the interpreter lock the eight
    worker threads need between their library calls.)"""
    __slots__ = ("host", "A", "b", "c", "m", "n", "factor", "order_info", "perm", "ub", "dense_cols", "unsplit_info")


def _upper_bounds(ub, n):
    """Host check of native upper bounds -> float64 (n,) with +inf where x_j is unbounded, or None when no entry is finite
    (the unbounded code runs exactly then).  ValueError for a wrong length, NaN or a negative entry."""
    if ub is None:
        return None
    u = np.ascontiguousarray(np.asarray(ub, dtype=np.float64).reshape(-1))
    if u.shape[0] != n:
        raise ValueError("ub has length %d, expected %d" % (u.shape[0], n))
    if np.isnan(u).any():
        raise ValueError("ub has NaN entries")
    if (u < 0).any():
        raise ValueError("ub has negative entries (0 <= x <= ub; shift lower bounds first)")
    return u if np.isfinite(u).any() else None


def _apply_row_order(A, b, perm):           # sparse A and b with device row i = caller's row perm[i]
    A = _sp.csc_matrix(_sp.csr_matrix(A)[perm])
    A.sort_indices()
    return A, np.ascontiguousarray(b[perm])


def _split_factor_path(P, A, factor, dense_cols):
    """The factor rule of prepare under dense_cols -> (path, perm, info); sets P.dense_cols (and P.unsplit_info, the ipm_order_rows
    record of the unsplit A, where the host ordered both)."""
    auto = isinstance(dense_cols, str)
    if auto and dense_cols != "auto":
        raise ValueError('dense_cols must be None, "auto" or a sequence of column indices, not %r' % (dense_cols,))
    cols = None if auto else check_dense_cols(dense_cols, P.n)
    if cols is not None and (not _is_sparse(A) or factor == "dense" or P.m <= FUSED_SMALL_MAX_ROWS):
        if cols.size:
            raise ValueError("dense_cols needs a sparse A of more than %d rows on the sparse factor" % FUSED_SMALL_MAX_ROWS)
        P.dense_cols = cols          # the empty set: IpmSolver clears the handle's set explicitly (ipm_set_dense_columns(h, 0, NULL))
        return _factor_path(A, P.m, factor)
    if auto:
        path = _factor_path(A, P.m, factor)
        if path[0] == "sparse" or not _is_sparse(A) or factor == "dense" or P.m <= FUSED_SMALL_MAX_ROWS:
            return path
        cols = dense_columns(A)
        if not cols.size:
            return path
        P.unsplit_info = path[2]
    elif not cols.size:
        P.dense_cols = cols
        return _factor_path(A, P.m, factor)
    split = _factor_path(without_columns(A, cols), P.m, factor)
    if split[0] == "sparse":
        P.dense_cols = cols
        return split
    if auto:
        return path
    raise ValueError("dense_cols: A without these columns does not go on the sparse factor (factor=%r)" % (factor,))


def prepare(A, b, c, dense=False, reorder="auto", factor=None, ub=None, dense_cols=None):
    """Host-only part of IpmSolver.__init__ (no device is touched) -> Prepared.  ub: native upper bounds (see IpmSolver).
    dense_cols: None (default) no split; a sequence of column indices: those columns are split out of the sparse
    factor, the factor rule and the row order see A without them, and the LP must end on the sparse factor (ValueError otherwise:
    the option is never dropped); "auto": the split is taken only where the factor rule puts A on the dense path and A without
    dense_columns(A) on the sparse factor.  P.dense_cols is the set in effect, or None (an empty array for an empty sequence)."""
    P = Prepared()
    if _is_sparse(A):
        A = _sp.csc_matrix(A, dtype=np.float64)
        A.sum_duplicates()
        A.sort_indices()
        m, n = A.shape
        if dense or A.nnz == 0:
            A = np.ascontiguousarray(A.toarray())
    else:
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        if A.ndim != 2:
            raise ValueError("A must be 2-D")
        m, n = A.shape
    P.m, P.n = int(m), int(n)
    b = _col(b, P.m, "b")
    c = _col(c, P.n, "c")
    P.ub = _upper_bounds(ub, P.n)
    P.host = (A, b, c)
    # factor: "dense" = blocked dense-tile Cholesky (tile envelope, RCM row order), "sparse" = multifrontal sparse
    # Cholesky (minimum-degree row order), "auto" (default; environment IPM_FACTOR overrides) = whichever the model
    # of prefer_sparse_factor expects to be faster
    factor = _factor_arg(factor)
    if factor not in ("auto", "dense", "sparse"):
        raise ValueError("factor must be 'auto', 'dense' or 'sparse'")
    P.dense_cols, P.unsplit_info = None, None
    if dense_cols is None:
        P.factor, P.perm, P.order_info = _factor_path(A, P.m, factor)
    else:
        P.factor, P.perm, P.order_info = _split_factor_path(P, A, factor, dense_cols)
    if factor == "sparse" and P.perm is None and _is_sparse(A):
        raise ValueError("factor='sparse': A A^T is too dense for the sparse factor (ipm_order_rows)")
    if P.perm is None and _is_sparse(A) and reorder and (reorder == "rcm" or P.m >= REORDER_MIN_ROWS):
        P.perm = envelope_row_order(A, force=(reorder == "rcm"))     # "auto": only when it pays
    if P.perm is not None:
        A, b = _apply_row_order(A, b, P.perm)
    P.A, P.b, P.c = A, b, c
    return P
