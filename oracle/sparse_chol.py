"""ctypes front of oracle/sparse_chol_oracle.cpp -- TEST INFRASTRUCTURE ONLY (tests/, smoke): the sequential CPU
restatement of the multifrontal sparse Cholesky of csrc/sparse_chol.h.  Built by __graft_entry__.build()."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsparse_chol_oracle.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB_PATH)
    return _lib


def factor_solve(A, d, rhs, eps=1e-30, big=1e64, shift_rel=0.0, wcap=32, lds=7680, want_factor=True):
    """Sparse Cholesky of A diag(d) A^T in the minimum-degree row order + one solve.  Returns dict(perm, L (dense, permuted
    order, or None), z (caller's row order), fixed, stats)."""
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    m, n = A.shape
    pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    perm = np.zeros(m, dtype=np.int32)
    L = np.zeros((m, m)) if want_factor else None
    z = np.zeros(m)
    nf = C.c_int(0)
    st = np.zeros(8)
    ip = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ii = np.ascontiguousarray(A.indices, dtype=np.int32)
    dv = np.ascontiguousarray(A.data, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    rc = load().spchol_oracle(m, n, ip.ctypes.data_as(pi), ii.ctypes.data_as(pi), dv.ctypes.data_as(pd), d.ctypes.data_as(pd),
                              rhs.ctypes.data_as(pd), C.c_double(eps), C.c_double(big), C.c_double(shift_rel), wcap, lds,
                              perm.ctypes.data_as(pi), L.ctypes.data_as(pd) if want_factor else None, z.ctypes.data_as(pd),
                              C.byref(nf), st.ctypes.data_as(pd))
    if rc:
        raise RuntimeError("spchol_oracle failed with code %d" % rc)
    keys = ("panels", "height", "widest_front", "factor_entries", "update_entries", "flops", "fan_in_nodes", "max_children")
    return dict(perm=perm.astype(np.int64), L=L, z=z, fixed=nf.value, stats=dict(zip(keys, st)))


def panel_table(A, wcap=32, lds=7680, relax=1.0):
    """The panel tree the device walks for A (csrc/sparse_symbolic.h: order_rows, then analyse with the product's settings)
    -> dict(perm (new -> old), c0, w, r, nchild, parent, rows): int64 arrays with one entry per node, fan-in nodes (w = 0)
    included, children before parents; rows: per node the array of its r rows in device order (own columns first)."""
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    m, n = A.shape
    pi = C.POINTER(C.c_int32)
    ip = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ii = np.ascontiguousarray(A.indices, dtype=np.int32)
    cnt = np.zeros(2, dtype=np.int32)
    fn = load().sppanel_table
    rc = fn(m, n, ip.ctypes.data_as(pi), ii.ctypes.data_as(pi), wcap, lds, C.c_double(relax), cnt.ctypes.data_as(pi), None, None, None)
    if rc:
        raise RuntimeError("sppanel_table failed with code %d" % rc)
    perm = np.zeros(m, dtype=np.int32)
    tab = np.zeros((int(cnt[0]), 5), dtype=np.int32)
    rows = np.zeros(max(1, int(cnt[1])), dtype=np.int32)
    rc = fn(m, n, ip.ctypes.data_as(pi), ii.ctypes.data_as(pi), wcap, lds, C.c_double(relax), cnt.ctypes.data_as(pi),
            perm.ctypes.data_as(pi), tab.ctypes.data_as(pi), rows.ctypes.data_as(pi))
    if rc:
        raise RuntimeError("sppanel_table failed with code %d" % rc)
    tab = tab.astype(np.int64)
    ends = np.cumsum(tab[:, 2])
    rows = [rows[e - r:e].astype(np.int64) for e, r in zip(ends, tab[:, 2])]
    return dict(perm=perm.astype(np.int64), c0=tab[:, 0], w=tab[:, 1], r=tab[:, 2], nchild=tab[:, 3], parent=tab[:, 4], rows=rows)


def symbolic_structures(A, wcap=32, lds=7680):
    """(perm, etree parent, entries per column of L) as csrc/sparse_symbolic.h computes them (amalgamation off), for
    the independent NumPy check of tests/test_sparse_symbolic.py."""
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    m, n = A.shape
    pi = C.POINTER(C.c_int32)
    perm, parent, cnt = (np.zeros(m, dtype=np.int32) for _ in range(3))
    ip = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ii = np.ascontiguousarray(A.indices, dtype=np.int32)
    rc = load().spsym_structures(m, n, ip.ctypes.data_as(pi), ii.ctypes.data_as(pi), wcap, lds, perm.ctypes.data_as(pi),
                                 parent.ctypes.data_as(pi), cnt.ctypes.data_as(pi))
    if rc:
        raise RuntimeError("spsym_structures failed with code %d" % rc)
    return perm.astype(np.int64), parent.astype(np.int64), cnt.astype(np.int64)
