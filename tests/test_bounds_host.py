"""Native upper bounds on the host (no GPU): the NumPy restatement of the bounded iteration (tests/bounds_oracle.py)
against scipy's HiGHS, general_form.native_form against the fixtures' own conversion, and the host-side checks of ub."""
import glob
import os

import numpy as np
import pytest
from scipy import sparse

from interiorpointmethod_amd import general_form as G
from interiorpointmethod_amd import solver as S

import bounds_oracle as BO

GEN = os.path.join(os.path.dirname(__file__), "golden", "general")
BOUNDED = [os.path.basename(f)[:-4] for f in sorted(glob.glob(os.path.join(GEN, "*.npz")))
           if np.isfinite(np.load(f)["ub"]).any()]


def load(name):
    z = np.load(os.path.join(GEN, name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    args = dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])
    return z, mat, args


def test_bounded_fixture_count():
    assert len(BOUNDED) == 27                      # of the 72 general-form files


@pytest.mark.parametrize("name", ["KB2", "BOEING2", "BORE3D", "FORPLAN", "STANDATA", "GROW7"])
def test_oracle_reaches_highs_optimum(name):
    from scipy.optimize import linprog
    _, _, args = load(name)
    F = G.native_form(**args)
    lp = BO.BoundedLP(F.A, F.b, F.c, F.u)
    x, y, s, w, z, info = lp.solve(tol=1e-9, tol_gap=1e-9, max_iter=200, state=BO.mehrotra_start(F.A, F.b, F.c, F.u))
    assert info["status"] == "converged"
    bnds = [(0.0, None if not np.isfinite(v) else float(v)) for v in F.u]
    ref = linprog(F.c.ravel(), A_eq=F.A, b_eq=F.b.ravel(), bounds=bnds, method="highs")
    assert ref.status == 0
    assert abs(info["objective"] - ref.fun) <= 1e-6 * max(1.0, abs(ref.fun))
    assert np.all(x > 0) and np.all(x[lp.U] < F.u[lp.U] + 1e-7 * (1 + F.u[lp.U]))
    # the original variables and the offset give the original objective
    xo = F.x_original(x)
    c = np.asarray(args["c"], dtype=np.float64).ravel()
    assert abs(c @ xo - (info["objective"] + F.offset)) <= 1e-9 * max(1.0, abs(c @ xo))
    assert abs(info["objective"] + F.offset - float(np.load(os.path.join(GEN, name + ".npz"))["netlib_optimum"])) <= \
        1e-6 * max(1.0, abs(ref.fun + F.offset))


@pytest.mark.parametrize("name", BOUNDED)
def test_native_form_matches_fixture_conversion(name):
    z, mat, args = load(name)
    F = G.native_form(**args)
    A0 = mat("std0_A")
    b0 = np.asarray(z["std0_b"], dtype=np.float64).ravel()
    n = np.asarray(args["c"]).size
    lb = np.asarray(args["lb"], dtype=np.float64).ravel()
    ub = np.asarray(args["ub"], dtype=np.float64).ravel()
    N = A0.shape[1]
    lb0 = np.concatenate([lb, np.zeros(N - n)])
    fixed = np.nonzero(lb == ub)[0]
    assert np.array_equal(F.fixed, fixed)
    assert F.A.shape == (A0.shape[0], N - fixed.size)                 # order m: no bound rows
    assert abs(F.A - A0[:, F.keep]).max() == 0.0
    assert np.allclose(F.b.ravel(), b0 - A0 @ lb0, rtol=0, atol=1e-12 * (1 + np.abs(b0).max()))
    u_full = np.concatenate([ub - lb, np.full(N - n, np.inf)])
    assert np.array_equal(F.u, u_full[F.keep])
    assert np.array_equal(F.c.ravel(), np.asarray(z["std0_c"]).ravel()[F.keep])
    # x' = 0 maps to x = lb with objective c^T lb = offset
    x0 = F.x_original(np.zeros(F.A.shape[1]))
    assert np.array_equal(x0, lb)
    assert F.offset == pytest.approx(float(np.asarray(args["c"]).ravel() @ lb), rel=1e-15, abs=0.0)
    # the folded form keeps one row per finite bound: the native order is that many rows smaller
    Af = mat("std_A")
    assert Af.shape[0] - F.A.shape[0] == int(np.isfinite(ub).sum())


def test_native_form_rejects_bad_bounds():
    _, _, args = load("KB2")
    bad = np.asarray(args["ub"], dtype=np.float64).copy()
    lb = np.zeros_like(bad)
    lb[3] = 5.0
    bad[3] = 4.0
    with pytest.raises(ValueError, match="ub < lb"):
        G.native_form(**dict(args, lb=lb, ub=bad))
    lb2 = np.zeros_like(bad)
    lb2[0] = -np.inf
    with pytest.raises(ValueError, match="-inf"):
        G.native_form(**dict(args, lb=lb2))
    with pytest.raises(ValueError, match="bounds"):
        G.new_interior_sparse(**args, bounds="sideways")


@pytest.mark.parametrize("ub", [np.array([1.0, -1.0, np.inf]), np.array([1.0, np.nan, 2.0]), np.array([1.0, 2.0])])
def test_solver_rejects_bad_ub_without_a_device(ub):
    A = np.array([[1.0, 1.0, 1.0]])
    with pytest.raises(ValueError):
        S.prepare(A, [1.0], [1.0, 2.0, 3.0], ub=ub)
    with pytest.raises(ValueError):                    # before any library or device call
        S.IpmSolver(A, [1.0], [1.0, 2.0, 3.0], ub=ub, use_torch=False, device=10 ** 6)


def test_all_infinite_ub_is_no_bound():
    P = S.prepare(np.array([[1.0, 1.0]]), [1.0], [1.0, 2.0], ub=[np.inf, np.inf])
    assert P.ub is None
    P = S.prepare(np.array([[1.0, 1.0]]), [1.0], [1.0, 2.0], ub=[np.inf, 3.0])
    assert P.ub[1] == 3.0 and np.isinf(P.ub[0])


def test_oracle_reduces_to_unbounded_iteration():
    """With no finite bound the restatement is the unbounded iteration of oracle/ipm_oracle.py."""
    from oracle import ipm_oracle as O
    A, b, c = O.synthetic_lp(20, 50, seed=3)
    lp = BO.BoundedLP(A, b, c, np.full(50, np.inf))
    x, y, s, w, z = lp.start(y0=0.0)
    xo, yo, so = O.initial_point(20, 50, y0=0.0)
    for _ in range(3):
        x, y, s, w, z, _ = lp.iterate(x, y, s, w, z)
        xo, yo, so, _ = O.iterate(A, b, c, xo, yo, so)
        assert np.allclose(x, np.ravel(xo), rtol=1e-12, atol=1e-14) and np.allclose(s, np.ravel(so), rtol=1e-12, atol=1e-14)
        assert not w.any() and not z.any()
