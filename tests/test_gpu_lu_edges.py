"""The device LU (csrc/getrf_f64.h; ipm_lu_solve / ipm_lu_factor) where it can go wrong without test_gpu_lu.py noticing:
both panel widths (IPM_LU_NB = 64 and 128: different instantiations of every kernel) over block boundaries, exact pivot
ties (the smaller row wins, across workgroups), more than LU_RC = 8 right-hand sides (more than one substitution group),
leading dimensions (pitched copies), power-of-two scaling and a subnormal pivot, and the first use of a width from two
threads at once.  References: exact arithmetic where the answer is exact, otherwise LAPACK and residuals in long double."""
import ctypes as C
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import scipy.linalg

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
ERR_INVALID_ARG = -1                                    # include/ipm_hip.h: IPM_ERR_INVALID_ARG
NAN_FILL = np.int64(0x7FF8DEADBEEF0001)                 # a quiet NaN with a payload: padding must come back bit for bit
BOUNDARY = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000, 4100]
SIZES_GPU_LU = [1, 2, 63, 64, 65, 127, 128, 129, 500, 1000, 2049, 4100]   # test_gpu_lu.SIZES: already run at width 64


@pytest.fixture(params=[64, 128], ids=["nb64", "nb128"])
def nb(request, monkeypatch):
    """The panel width: lu_nb() reads IPM_LU_NB on every call."""
    monkeypatch.setenv("IPM_LU_NB", str(request.param))
    return request.param


def _p(a):
    return a.ctypes.data_as(PD)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def backward_error(A, x, b):
    """test_gpu_lu.backward_error with the residual in long double: ||A x - b|| / (||A|| ||x|| n eps), infinity norms,
    worst right-hand side.  A and x may be long double already (column-scaled systems)."""
    n = A.shape[0]
    X, B = np.asarray(x).reshape(n, -1), np.asarray(b).reshape(n, -1)
    Xl = X.astype(np.longdouble)
    r = np.zeros(X.shape[1], dtype=np.longdouble)
    for i in range(0, n, 512):                           # row blocks: a long double copy of all of A would be large
        R = A[i:i + 512].astype(np.longdouble) @ Xl - B[i:i + 512]
        r = np.maximum(r, np.abs(R).max(axis=0))
    nA = np.abs(A.astype(np.longdouble)).sum(axis=1).max()
    xm = np.maximum(np.abs(Xl).max(axis=0), np.longdouble(1e-300))
    return float(np.max(r / (nA * xm * n * EPS)))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def well_conditioned(n, seed):
    """Gaussian plus a scaled random permutation (test_gpu_lu.well_conditioned): continuous draws, so every pivot column
    has a unique maximum, and partial pivoting has to move rows."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A[np.arange(n), rng.permutation(n)] += 2.0 * np.sqrt(n)
    return A


def solve_packed(A, B):
    n, k = B.shape
    X = np.empty_like(B)
    info = C.c_int64(-1)
    rc = _lib.load().ipm_lu_solve(0, n, _p(A), n, k, _p(B), k, _p(X), k, C.byref(info))
    assert rc == _lib.IPM_OK and info.value == 0, (rc, info.value)
    return X


def padded(M, ld):
    out = np.empty((M.shape[0], ld))
    bits(out)[...] = NAN_FILL
    out[:, :M.shape[1]] = M
    return out


# ---------------------------------------------------------------------------------------------- A. block boundaries

@pytest.mark.parametrize("nb_,n", [(128, n) for n in BOUNDARY] + [(64, n) for n in BOUNDARY if n not in SIZES_GPU_LU])
def test_boundary_sizes(monkeypatch, nb_, n):
    monkeypatch.setenv("IPM_LU_NB", str(nb_))
    rng = np.random.default_rng(7000 + n)
    A = well_conditioned(n, n + 1)
    b = rng.standard_normal((n, 3))
    x = ipm.lu_solve(A, b)
    assert rel(x, np.linalg.solve(A, b)) <= 1e-10, (nb_, n)
    assert backward_error(A, x, b) <= 10.0, (nb_, n)
    G = rng.standard_normal((n, n))                     # plain Gaussian: unsymmetric, indefinite, larger growth
    assert backward_error(G, ipm.lu_solve(G, b), b) <= 10.0, (nb_, n)
    LU, piv = ipm.lu_factor(A)
    LUs, pivs = scipy.linalg.lu_factor(A)
    assert np.array_equal(piv, pivs), (nb_, n, np.flatnonzero(piv != pivs)[:8])
    assert rel(LU, LUs) <= 1e-12, (nb_, n, rel(LU, LUs))


# ---------------------------------------------------------------------------------------------- B. exact pivot ties

def sylvester(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


@lru_cache(maxsize=None)
def _hadamard(n, signed):
    """H_n, with random +-1 row and column signs when `signed`, and scipy's LU of it (the CPU premise checked here)."""
    A = sylvester(n)
    if signed:
        rng = np.random.default_rng(n)
        A = A * rng.choice([-1.0, 1.0], n)[:, None] * rng.choice([-1.0, 1.0], n)[None, :]
    LUs, pivs = scipy.linalg.lu_factor(A)
    return A, LUs, pivs


@pytest.mark.parametrize("signed", [False, True], ids=["plain", "signed"])
@pytest.mark.parametrize("n", [64, 128, 256, 1024, 4096])
def test_hadamard_exact_ties(nb, n, signed):
    """GEPP on a Hadamard matrix ties every column across all rows below the diagonal (rows of different workgroups too);
    the smaller row wins, so no interchange happens.  Every entry of L and U is 0 or +-2^k (|.| <= n) and every partial
    sum is an integer below 2^53, so any summation order is exact: LU equals LAPACK's exactly, and A^-1 = A^T / n."""
    A, LUs, pivs = _hadamard(n, signed)
    nz = np.abs(LUs[LUs != 0.0])
    assert np.array_equal(pivs, np.arange(n))                           # the premise, on the CPU
    assert np.all(np.frexp(nz)[0] == 0.5) and nz.max() <= n
    LU, piv = ipm.lu_factor(A)
    assert np.array_equal(piv, np.arange(n)), np.flatnonzero(piv != np.arange(n))[:8]
    assert np.array_equal(LU, LUs), np.argwhere(LU != LUs)[:8]
    b = np.random.default_rng(n + signed).integers(-8, 9, size=(n, 2)).astype(np.float64)
    exact = (A.T.astype(np.int64) @ b.astype(np.int64)) / n            # exact: integers over a power of two
    assert np.array_equal(scipy.linalg.lu_solve((LUs, pivs), b), exact)  # the premise, on the CPU
    assert np.array_equal(ipm.lu_solve(A, b), exact)


@pytest.mark.parametrize("n", [64, 129, 200, 1000, 1024])
def test_wilkinson_growth_matrix(nb, n):
    """1 on the diagonal, -1 below it, 1 in the last column: every column below the diagonal stays exactly -1 and ties the
    diagonal 1, so no interchange; L is -1 below the diagonal, U the identity except its last column 2^i (2^1023 at
    n = 1024, still finite).  That column only to 1e-14: a blocked update's partial sums of powers of two can round."""
    W = np.eye(n) - np.tril(np.ones((n, n)), -1)
    W[:, -1] = 1.0
    LU, piv = ipm.lu_factor(W)
    assert np.array_equal(piv, np.arange(n))
    assert np.all(LU[np.tril_indices(n, -1)] == -1.0)
    assert np.all(np.diag(LU)[:-1] == 1.0)
    assert np.all(np.triu(LU, 1)[:, :-1] == 0.0)
    last = np.ldexp(1.0, np.arange(n))
    assert np.all(np.isfinite(LU[:, -1]))
    assert np.max(np.abs(LU[:, -1] - last) / last) <= 1e-14


@lru_cache(maxsize=None)
def _first_column_tie():
    n = 4100
    A = well_conditioned(n, 4100)
    M = np.abs(A[:, 0]).max() + 1.0
    A[3000, 0], A[70, 0], A[700, 0] = M, -M, M          # three rows tie for the first pivot, in different workgroups
    LUs, pivs = scipy.linalg.lu_factor(A)
    return A, LUs, pivs


def test_first_column_tie_across_workgroups(nb):
    A, LUs, pivs = _first_column_tie()
    assert pivs[0] == 70                                # LAPACK idamax: the first of the tied rows
    LU, piv = ipm.lu_factor(A)
    assert piv[0] == 70
    assert np.array_equal(piv, pivs), np.flatnonzero(piv != pivs)[:8]
    assert rel(LU, LUs) <= 1e-12


# ---------------------------------------------------------------------------------------------- C. many right-hand sides

@pytest.mark.parametrize("n", [65, 300, 1000])
def test_many_rhs_metamorphic(nb, n):
    """Every right-hand side is solved with the same arithmetic whichever substitution group (LU_RC = 8 per group) and
    position it lands in: a column of an nrhs = k solve equals the nrhs = 1 solve of that column bit for bit, and
    permuting the columns of B permutes X bit for bit."""
    rng = np.random.default_rng(n)
    A = well_conditioned(n, 3 * n)
    B = rng.standard_normal((n, 100))
    single = [solve_packed(A, B[:, [q]]) for q in range(B.shape[1])]
    for k in (8, 9, 16, 17, 37, 100):
        X = solve_packed(A, np.ascontiguousarray(B[:, :k]))
        for q in range(k):
            assert same_bits(X[:, [q]], single[q]), (k, q)
        perm = rng.permutation(k)
        Xp = solve_packed(A, np.ascontiguousarray(B[:, perm]))
        assert same_bits(Xp, np.ascontiguousarray(X[:, perm])), k
        assert backward_error(A, X, B[:, :k]) <= 10.0, k


# ---------------------------------------------------------------------------------------------- D. leading dimensions

@pytest.mark.parametrize("n,nrhs", [(65, 1), (65, 9), (300, 1), (300, 9)])
def test_leading_dimensions(nb, n, nrhs):
    lib = _lib.load()
    rng = np.random.default_rng(n * 100 + nrhs)
    A = well_conditioned(n, n + 5)
    B = rng.standard_normal((n, nrhs))
    Xref = solve_packed(A, B)
    lda, ldb, ldlu = n + 3, nrhs + 5, n + 7
    Ap, Bp = padded(A, lda), padded(B, ldb)
    Ap0, Bp0 = Ap.copy(), Bp.copy()
    Xp = padded(np.empty((n, 0)), ldb)
    info = C.c_int64(-1)
    rc = lib.ipm_lu_solve(0, n, _p(Ap), lda, nrhs, _p(Bp), ldb, _p(Xp), ldb, C.byref(info))
    assert rc == _lib.IPM_OK and info.value == 0
    assert same_bits(np.ascontiguousarray(Xp[:, :nrhs]), Xref)
    assert np.all(bits(Xp)[:, nrhs:] == NAN_FILL)        # the padding of X is not written
    assert same_bits(Ap, Ap0) and same_bits(Bp, Bp0)    # the inputs are not written
    XB = Bp.copy()                                      # X aliases B, ldx == ldb > nrhs
    rc = lib.ipm_lu_solve(0, n, _p(Ap), lda, nrhs, _p(XB), ldb, _p(XB), ldb, C.byref(info))
    assert rc == _lib.IPM_OK and info.value == 0
    assert same_bits(np.ascontiguousarray(XB[:, :nrhs]), Xref)
    assert np.all(bits(XB)[:, nrhs:] == NAN_FILL)
    LUref, pivref = ipm.lu_factor(A)
    LUp = padded(np.empty((n, 0)), ldlu)
    piv = np.full(n, -5, dtype=np.int32)
    rc = lib.ipm_lu_factor(0, n, _p(Ap), lda, _p(LUp), ldlu, piv.ctypes.data_as(PI), C.byref(info))
    assert rc == _lib.IPM_OK and info.value == 0
    assert same_bits(np.ascontiguousarray(LUp[:, :n]), LUref) and np.array_equal(piv, pivref)
    assert np.all(bits(LUp)[:, n:] == NAN_FILL)
    X = np.empty((n, ldb))
    for args in [(n - 1, nrhs, ldb, ldb), (lda, nrhs, nrhs - 1, ldb), (lda, nrhs, ldb, nrhs - 1)]:
        la, k, lb, lx = args
        rc = lib.ipm_lu_solve(0, n, _p(Ap), la, k, _p(Bp), lb, _p(X), lx, C.byref(info))
        assert rc == ERR_INVALID_ARG, args
    for la, ll in [(n - 1, ldlu), (lda, n - 1)]:
        rc = lib.ipm_lu_factor(0, n, _p(Ap), la, _p(LUp), ll, piv.ctypes.data_as(PI), C.byref(info))
        assert rc == ERR_INVALID_ARG, (la, ll)


# ---------------------------------------------------------------------------------------------- E. scaling

@pytest.mark.parametrize("n", [129, 300])
def test_power_of_two_column_scaling(nb, n):
    """Scaling by powers of two commutes with every rounding (no overflow or underflow here), and partial pivoting sees
    the same column order: lu_factor(A D) has A's pivots and L, and U D, bit for bit; solving A D x = b gives D^-1 x;
    scaling a right-hand side by 2^e scales its solution by 2^e."""
    rng = np.random.default_rng(n)
    A = well_conditioned(n, 11 * n)
    e = rng.integers(-600, 601, size=n)
    AD = np.ldexp(A, e[None, :])
    LU, piv = ipm.lu_factor(A)
    LUd, pivd = ipm.lu_factor(AD)
    assert np.array_equal(piv, pivd)
    assert same_bits(np.tril(LUd, -1), np.tril(LU, -1))
    assert same_bits(np.triu(LUd), np.ldexp(np.triu(LU), e[None, :]))
    B = rng.standard_normal((n, 3))
    X = ipm.lu_solve(A, B)
    assert same_bits(ipm.lu_solve(AD, B), np.ldexp(X, -e[:, None]))
    eb = rng.integers(-600, 601, size=3)
    assert same_bits(ipm.lu_solve(A, np.ldexp(B, eb[None, :])), np.ldexp(X, eb[None, :]))


@pytest.mark.parametrize("col", [0, 7])
def test_subnormal_pivot_column(nb, col):
    """One column scaled by 2^-1070: its entries, and the pivot of that column, are subnormal.  A flushed (denormals-are-
    zero) pivot would read as exactly zero and report a nonsingular matrix as singular.  The column must be final before
    anything is subtracted from it (column 0, or column 7 behind an upper-triangular leading block whose eliminations
    change nothing), since an update rounding in the subnormal range keeps only a few bits: LAPACK loses the column there
    too.  The right-hand side is scaled by 2^-100 so that x[col] ~ 2^970 is representable.  Backward error of the
    column-scaled system, long double residual."""
    n = 300
    rng = np.random.default_rng(300 + col)
    A = well_conditioned(n, 17 + col)
    if col:
        A[col:, :col] = 0.0
        A[:col, :col] = np.triu(A[:col, :col]) + np.diag(np.full(col, 2.0 * np.sqrt(n)))
    A[:, col] = np.ldexp(A[:, col], -1070)
    B = np.ldexp(rng.standard_normal((n, 2)), -100)
    X = np.empty_like(B)
    info = C.c_int64(-1)
    rc = _lib.load().ipm_lu_solve(0, n, _p(A), n, 2, _p(B), 2, _p(X), 2, C.byref(info))
    assert rc == _lib.IPM_OK, (rc, _lib.load().ipm_last_error(None))
    assert info.value == 0
    assert np.all(np.isfinite(X))
    LU, piv = ipm.lu_factor(A)
    assert 0.0 < abs(LU[col, col]) < np.finfo(np.float64).tiny            # the premise: the pivot is subnormal
    As = A.astype(np.longdouble)
    As[:, col] = np.ldexp(As[:, col], 1070)
    Xs = X.astype(np.longdouble)
    Xs[col] = np.ldexp(Xs[col], -1070)
    assert backward_error(As, Xs, B) <= 10.0


# ---------------------------------------------------------------------------------------------- F. two threads

_THREADS = r'''
import threading
import numpy as np
import interiorpointmethod_amd as ipm

n = 300
rng = np.random.default_rng(1)
A = [rng.standard_normal((n, n)) for _ in range(2)]
B = [rng.standard_normal((n, 3)) for _ in range(2)]
out, err = [None, None], [None, None]
go = threading.Barrier(2)

def work(i):
    try:
        go.wait()
        out[i] = ipm.lu_solve(A[i], B[i])
    except Exception as e:
        err[i] = repr(e)

ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
for t in ts:
    t.start()
for t in ts:
    t.join()
assert err == [None, None], err
for i in range(2):
    ref = ipm.lu_solve(A[i], B[i])
    assert np.array_equal(out[i].view(np.int64), ref.view(np.int64)), i
print("LU_THREADS_OK")
'''


@pytest.mark.parametrize("width", [64, 128])
def test_first_use_from_two_threads(width):
    """A fresh process whose first LU at this width is two concurrent lu_solve calls (the kernel attributes -- 128 KiB and
    136 KiB of dynamic LDS at width 128 -- are set on first use): both succeed and match their single-threaded results."""
    env = dict(os.environ, IPM_LU_NB=str(width), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", _THREADS], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0 and "LU_THREADS_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
