"""Host pieces of the general-matrix seam (no GPU): the unreduced KKT system method="kkt" assembles against the oracle's
(m + 2n) matrix, its right-hand sides reproduce the reference's method="full" directions with CPU LAPACK, and
ipm_lu_solve / ipm_lu_factor reject bad arguments before touching a device."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib, kkt, solver
from oracle import ipm_oracle as O


def _kat(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "kat_%s.npz" % name))
    A = sparse.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=tuple(int(v) for v in z["shape"]))
    return z, A


@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "BANDM"])
def test_kkt_matrix_matches_oracle(golden_dir, name):
    z, A = _kat(golden_dir, name)
    k = int(z["iters"][1])
    x, s = z["k%d_x" % k], z["k%d_s" % k]
    K = solver._kkt_matrix(A, x, s)
    Ko = O.kkt_matrix(A, x, s).toarray()
    assert np.array_equal(K, Ko)
    Kd = solver._kkt_matrix(A.toarray(), x, s)                    # the dense-A assembly is the same matrix
    assert np.array_equal(Kd, Ko)
    m, n = A.shape
    assert np.all(np.diag(K)[:n] == 0.0)                          # the zero block: needs pivoting


def test_kkt_assembly_sums_duplicates():
    A = sparse.coo_matrix(([1.0, 2.0, 3.0], ([0, 0, 1], [1, 1, 0])), shape=(2, 3))
    K = solver._kkt_matrix(A, np.ones(3), np.ones(3))
    assert K[3 + 0, 1] == 3.0 and K[1, 3 + 0] == 3.0 and K[3 + 1, 0] == 3.0


@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "BANDM"])
def test_kkt_rhs_reproduces_reference_full_with_lapack(golden_dir, name, monkeypatch):
    """The assembled systems (matrix + predictor / corrector right-hand sides), solved by CPU LAPACK in place of the
    device LU, give the reference's method="full" directions of the fixture at k = 0 and the middle iterate."""
    monkeypatch.setattr(kkt, "lu_solve", lambda K, rhs, device=0: np.linalg.solve(K, rhs))
    z, A = _kat(golden_dir, name)
    b, c = z["b"], z["c"]
    for k in (int(z["iters"][0]), int(z["iters"][1])):
        p = "k%d_" % k
        x, y, s = z[p + "x"], z[p + "y"], z[p + "s"]
        got = ipm.direction_predicted_sparse(A, b, c, x, y, s, method="kkt")
        for g, nm in zip(got, ("dxa", "dya", "dsa")):
            assert g.shape == z[p + nm].shape
            assert np.linalg.norm(g - z[p + nm]) <= 1e-11 * max(1.0, np.linalg.norm(z[p + nm])), (name, k, nm)
        got = ipm.direction_corrected_sparse(A, b, c, x, y, s, z[p + "dxa"], z[p + "dya"], z[p + "dsa"], method="kkt")
        for g, nm in zip(got, ("dx", "dy", "ds")):
            assert np.linalg.norm(g - z[p + nm]) <= 1e-10 * max(1.0, np.linalg.norm(z[p + nm])), (name, k, nm)


def test_kkt_corrector_needs_the_affine_direction(golden_dir):
    z, A = _kat(golden_dir, "AFIRO")
    with pytest.raises(ValueError):
        ipm.direction_corrected_sparse(A, z["b"], z["c"], z["k0_x"], z["k0_y"], z["k0_s"], method="kkt")
    with pytest.raises(ValueError):
        ipm.direction_predicted_sparse(A, z["b"], z["c"], z["k0_x"], z["k0_y"], z["k0_s"], method="eliminate")


def test_lu_entry_points_reject_bad_arguments(built_lib):
    lib = ipm.load_library()
    pd = C.POINTER(C.c_double)
    A = np.eye(4)
    B = np.ones((4, 2))
    X = np.empty((4, 2))
    info = C.c_int64(0)
    P = lambda a: a.ctypes.data_as(pd)                            # noqa: E731
    for n, lda, nrhs, ldb, ldx in [(0, 4, 2, 2, 2), (4, 3, 2, 2, 2), (4, 4, 0, 2, 2), (4, 4, 2, 1, 2), (4, 4, 2, 2, 1)]:
        assert lib.ipm_lu_solve(0, n, P(A), lda, nrhs, P(B), ldb, P(X), ldx, C.byref(info)) == -1
        assert b"bad arguments" in lib.ipm_last_error(None)
    assert lib.ipm_lu_solve(0, 4, None, 4, 2, P(B), 2, P(X), 2, C.byref(info)) == -1
    LU = np.empty((4, 4))
    piv = np.empty(4, dtype=np.int32)
    pi = piv.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ipm_lu_factor(0, 4, P(A), 3, P(LU), 4, pi, C.byref(info)) == -1
    assert lib.ipm_lu_factor(0, 4, P(A), 4, P(LU), 3, pi, C.byref(info)) == -1
    assert lib.ipm_lu_factor(0, 4, P(A), 4, P(LU), 4, None, C.byref(info)) == -1
    assert _lib.ERR_SINGULAR == -7


def test_lu_no_cpu_fallback_without_device(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises((ipm.IpmError, ipm.IpmLibraryError)):
        ipm.solve_linear(np.array([[0.0, 1.0], [1.0, 0.0]]), np.ones(2), method="lu")
    with pytest.raises(ValueError):
        ipm.lu_solve(np.ones((2, 3)), np.ones(2))
