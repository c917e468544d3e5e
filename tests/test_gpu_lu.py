"""The general-matrix seam on the device: LU with partial pivoting (csrc/getrf_f64.h; ipm_lu_solve / ipm_lu_factor) against
LAPACK, and the reference's unreduced KKT direction (method="kkt") against its method="full" fixtures."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import scipy.linalg
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, solver

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 500, 1000, 2049, 4100]


def backward_error(A, x, b):
    """||A x - b|| / (||A|| ||x|| n eps), infinity norms, worst right-hand side."""
    n = A.shape[0]
    X, B = x.reshape(n, -1), b.reshape(n, -1)
    r = np.abs(A @ X - B).max(axis=0)
    nA = np.abs(A).sum(axis=1).max()
    return float(np.max(r / (nA * np.maximum(np.abs(X).max(axis=0), 1e-300) * n * EPS)))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def well_conditioned(n, seed):
    """Gaussian plus a scaled random permutation: well conditioned, and partial pivoting has to move rows."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A[np.arange(n), rng.permutation(n)] += 2.0 * np.sqrt(n)
    return A


def _kat(name):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_%s.npz" % name))
    A = sparse.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=tuple(int(v) for v in z["shape"]))
    return z, A


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nrhs", [1, 7])
def test_lu_solve_general_matrices(n, nrhs):
    rng = np.random.default_rng(1000 * n + nrhs)
    b = rng.standard_normal((n, nrhs)) if nrhs > 1 else rng.standard_normal(n)
    A = well_conditioned(n, n)
    x = ipm.solve_linear(A, b, method="lu")
    assert x.shape == b.shape
    assert rel(x, np.linalg.solve(A, b)) <= 1e-10, n
    assert backward_error(A, x, b) <= 10.0
    G = rng.standard_normal((n, n))                    # plain Gaussian: unsymmetric, indefinite
    x = ipm.lu_solve(G, b)
    assert backward_error(G, x, b) <= 10.0
    P = np.eye(n)[rng.permutation(n)]                  # a permuted identity: zero diagonal (n > 1)
    x = ipm.lu_solve(P, b)
    assert np.array_equal(x, np.linalg.solve(P, b))


def test_lu_solve_shapes_and_sparse_input():
    A = well_conditioned(40, 3)
    b = np.arange(40.0)
    for bb in (b, b.reshape(-1, 1), np.stack([b, -b, 2 * b], axis=1)):
        x = ipm.solve_linear(sparse.csr_matrix(A), bb, method="lu")
        assert x.shape == np.linalg.solve(A, bb).shape
        assert rel(x, np.linalg.solve(A, bb)) <= 1e-12


@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "BANDM"])
def test_lu_solve_kkt_matrix(name):
    """The reference's unreduced KKT matrix (zero diagonal block) at the fixture's middle iterate."""
    z, A = _kat(name)
    k = int(z["iters"][1])
    K = solver._kkt_matrix(A, z["k%d_x" % k], z["k%d_s" % k])
    rng = np.random.default_rng(7)
    for nrhs in (1, 7):
        b = rng.standard_normal((K.shape[0], nrhs))
        x = ipm.lu_solve(K, b)
        assert backward_error(K, x, b) <= 10.0, name


@pytest.mark.parametrize("n", [5, 64, 130, 300, 1000])
def test_lu_factor_matches_scipy(n):
    A = np.random.default_rng(n).standard_normal((n, n))     # continuous draws: every pivot column has a unique maximum
    LU, piv = ipm.lu_factor(A)
    LUs, pivs = scipy.linalg.lu_factor(A)
    assert np.array_equal(piv, pivs)
    assert rel(LU, LUs) <= 1e-12
    P = np.arange(n)
    for i, p in enumerate(piv):
        P[[i, p]] = P[[p, i]]
    L = np.tril(LU, -1) + np.eye(n)
    U = np.triu(LU)
    assert np.abs(L @ U - A[P]).max() <= 50 * n * EPS * np.abs(A).max()


def test_singular_and_nonfinite():
    lib = ipm.load_library()
    pd = C.POINTER(C.c_double)
    n = 50
    A = np.random.default_rng(5).standard_normal((n, n))
    A[30] = A[12]                                         # a duplicated row: rank n - 1, the last pivot is zero
    b = np.ones(n)
    X = np.empty(n)
    info = C.c_int64(0)
    rc = lib.ipm_lu_solve(0, n, A.ctypes.data_as(pd), n, 1, b.ctypes.data_as(pd), 1, X.ctypes.data_as(pd), 1, C.byref(info))
    assert rc == _lib.ERR_SINGULAR and b"singular" in lib.ipm_last_error(None)
    # the two equal rows see identical updates (one panel: the same rank-1 steps), so once one of them is the pivot row the
    # other is exactly zero and stays below every non-zero row: the zero pivot is the last one
    assert info.value == n
    with pytest.warns(RuntimeWarning):
        LU, piv = ipm.lu_factor(A)
    assert LU[info.value - 1, info.value - 1] == 0.0
    assert np.all(np.diag(LU)[:info.value - 1] != 0.0)
    with pytest.raises(np.linalg.LinAlgError):
        ipm.solve_linear(A, b, method="lu")
    Zc = np.random.default_rng(6).standard_normal((300, 300))
    Zc[:, 200] = 0.0                                      # a zero column stays zero through every panel and trailing update
    with pytest.warns(RuntimeWarning):
        LU, piv = ipm.lu_factor(Zc)
    rc = lib.ipm_lu_solve(0, 300, Zc.ctypes.data_as(pd), 300, 1, np.ones(300).ctypes.data_as(pd), 1,
                          np.empty(300).ctypes.data_as(pd), 1, C.byref(info))
    assert rc == _lib.ERR_SINGULAR and info.value == 201
    assert LU[200, 200] == 0.0 and piv[200] == 200
    Z = np.zeros((3, 3))
    Z[0, 1] = Z[1, 0] = 1.0                               # column 2 is zero: info = 3
    rc = lib.ipm_lu_solve(0, 3, Z.ctypes.data_as(pd), 3, 1, b.ctypes.data_as(pd), 1, X.ctypes.data_as(pd), 1, C.byref(info))
    assert rc == _lib.ERR_SINGULAR and info.value == 3
    for bad in (np.nan, np.inf, -np.inf):
        Ab = np.eye(n)
        Ab[7, 3] = bad
        rc = lib.ipm_lu_solve(0, n, Ab.ctypes.data_as(pd), n, 1, b.ctypes.data_as(pd), 1, X.ctypes.data_as(pd), 1, C.byref(info))
        assert rc == _lib.ERR_INVALID_INPUT
        bb = np.ones(n)
        bb[4] = bad
        rc = lib.ipm_lu_solve(0, n, np.eye(n).ctypes.data_as(pd), n, 1, bb.ctypes.data_as(pd), 1, X.ctypes.data_as(pd), 1, C.byref(info))
        assert rc == _lib.ERR_INVALID_INPUT
        LU = np.empty((n, n))
        piv = np.empty(n, dtype=np.int32)
        rc = lib.ipm_lu_factor(0, n, Ab.ctypes.data_as(pd), n, LU.ctypes.data_as(pd), n,
                               piv.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info))
        assert rc == _lib.ERR_INVALID_INPUT and b"NaN or Inf" in lib.ipm_last_error(None)


def test_bitwise_repeatable_and_aliasing():
    lib = ipm.load_library()
    pd = C.POINTER(C.c_double)
    n, k = 777, 3
    rng = np.random.default_rng(11)
    A = rng.standard_normal((n, n))
    B = rng.standard_normal((n, k))
    x1, x2 = ipm.lu_solve(A, B), ipm.lu_solve(A, B)
    assert np.array_equal(x1, x2)
    (l1, p1), (l2, p2) = ipm.lu_factor(A), ipm.lu_factor(A)
    assert np.array_equal(l1, l2) and np.array_equal(p1, p2)
    XB = B.copy()                                         # X aliases B
    info = C.c_int64(0)
    rc = lib.ipm_lu_solve(0, n, A.ctypes.data_as(pd), n, k, XB.ctypes.data_as(pd), k, XB.ctypes.data_as(pd), k, C.byref(info))
    assert rc == 0 and info.value == 0
    assert np.array_equal(XB, x1)


@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "BANDM"])
def test_kkt_direction_matches_reference_full(name):
    """method="kkt" against the reference's method="full" outputs: 1e-11 at k = 0, 1e-8 at the middle iterate (predictor
    and corrector; the corrector is fed the fixture's affine direction)."""
    z, A = _kat(name)
    b, c = z["b"], z["c"]
    for k, tol in ((int(z["iters"][0]), 1e-11), (int(z["iters"][1]), 1e-8)):
        p = "k%d_" % k
        x, y, s = z[p + "x"], z[p + "y"], z[p + "s"]
        got = ipm.direction_predicted_sparse(A, b, c, x, y, s, method="kkt")
        for g, nm in zip(got, ("dxa", "dya", "dsa")):
            assert g.shape == z[p + nm].shape
            assert rel(g, z[p + nm]) <= tol, (name, k, nm, rel(g, z[p + nm]))
        got = ipm.direction_corrected_sparse(A, b, c, x, y, s, z[p + "dxa"], z[p + "dya"], z[p + "dsa"], method="kkt")
        for g, nm in zip(got, ("dx", "dy", "ds")):
            assert rel(g, z[p + nm]) <= tol, (name, k, nm, rel(g, z[p + nm]))


@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "BANDM"])
def test_kkt_direction_last_iterate(name):
    """At the last stored iterate the reference's LU is itself unstable (AFIRO k = 60: condition 2e38).  The device LU is
    compared with CPU LAPACK dgesv of the same assembled system, on the components where dgesv and the fixture agree within
    1e-3, with a bound of max(1e-8, 100 x that spread)."""
    z, A = _kat(name)
    k = int(z["iters"][2])
    p = "k%d_" % k
    x, y, s = z[p + "x"], z[p + "y"], z[p + "s"]
    _, _, _, rb, rc = solver._kkt_residuals(A, z["b"], z["c"], x, y, s)
    K = solver._kkt_matrix(A, x, s)
    m, n = A.shape
    ref = np.linalg.solve(K, np.concatenate([-rc, -rb, -(x.ravel() * s.ravel())]))
    ref = (ref[:n].reshape(-1, 1), ref[n:n + m].reshape(-1, 1), ref[n + m:].reshape(-1, 1))
    got = ipm.direction_predicted_sparse(A, z["b"], z["c"], x, y, s, method="kkt")
    checked = 0
    for g, r, nm in zip(got, ref, ("dxa", "dya", "dsa")):
        spread = rel(r, z[p + nm])
        if spread < 1e-3:
            checked += 1
            assert rel(g, r) <= max(1e-8, 100.0 * spread), (name, k, nm, spread, rel(g, r))
    if name != "AFIRO":
        assert checked == 3


@pytest.mark.parametrize("ex", ["ex1", "ex2", "ex3"])
def test_dense_kkt_direction_at_reference_start(golden_dir, ex):
    """dense_ex*.npz: the reference's dense direction_predicted at its start point x = s = 1, y = 0 (main.py:287-302)."""
    z = np.load(os.path.join(golden_dir, "dense_%s.npz" % ex))
    A = z["A"]
    m, n = A.shape
    x, y, s = np.ones((n, 1)), np.zeros((m, 1)), np.ones((n, 1))
    got = ipm.direction_predicted(A, z["b"], z["c"], x, y, s, method="kkt")
    for g, nm in zip(got, ("k0_dxa", "k0_dya", "k0_dsa")):
        assert rel(g, z[nm]) <= 1e-11, (ex, nm)
    got = ipm.direction_corrected(A, z["b"], z["c"], x, y, s, z["k0_dxa"], z["k0_dya"], z["k0_dsa"], method="kkt")
    for g, nm in zip(got, ("k0_dx", "k0_dy", "k0_ds")):
        assert rel(g, z[nm]) <= 1e-10, (ex, nm)


def test_kkt_order_20480():
    """One solve of the KKT order of the 4096 x 8192 headline LP (2n + m = 20480) at its start point; the backward error
    is asserted, the time printed."""
    from interiorpointmethod_amd.workloads import synthetic_lp
    A, b, c = synthetic_lp(4096, 8192, seed=0)
    m, n = A.shape
    x, y, s = np.ones((n, 1)), np.zeros((m, 1)), np.ones((n, 1))
    _, _, _, rb, rc = solver._kkt_residuals(A, b, c, x, y, s)
    K = solver._kkt_matrix(A, x, s)
    rhs = np.concatenate([-rc, -rb, -(x * s).ravel()])
    t0 = time.perf_counter()
    sol = ipm.lu_solve(K, rhs)
    t1 = time.perf_counter()
    Ks = sparse.csr_matrix(K)
    r = np.abs(Ks @ sol - rhs).max()
    nK = np.abs(Ks).sum(axis=1).max()
    be = r / (nK * np.abs(sol).max() * K.shape[0] * EPS)
    print("\n[lu 20480] wall %.3f s (upload + factor + solve + download), backward error %.3g" % (t1 - t0, be))
    assert be <= 10.0
