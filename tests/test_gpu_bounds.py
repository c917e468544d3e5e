"""Native upper bounds on the GPU: the bounded kernels of csrc/vector_ops.h and csrc/small_lp.h on every
launch chain, against the NumPy restatement of tests/bounds_oracle.py, dense LPs with a known optimum, the general-form
Netlib files, the roll-back of (w, z), bit-identity of the unbounded code and the lockstep refusal."""
import os

import numpy as np
import pytest
from scipy import sparse

from interiorpointmethod_amd import _lib
from interiorpointmethod_amd import general_form as G
from interiorpointmethod_amd import solver as S

import bounds_oracle as BO

pytestmark = pytest.mark.gpu

GEN = os.path.join(os.path.dirname(__file__), "golden", "general")
NETLIB = os.path.join(os.path.dirname(__file__), "golden", "netlib")


def load(name):
    z = np.load(os.path.join(GEN, name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return z, dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                   bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


def load_netlib(name):
    d = np.load(os.path.join(NETLIB, name + ".npz"))
    A = sparse.csc_matrix((d["data"], d["indices"], d["indptr"]), shape=tuple(int(v) for v in d["shape"]))
    return A, np.asarray(d["b"], dtype=np.float64).ravel(), np.asarray(d["c"], dtype=np.float64).ravel(), float(d["cTlb"])


def rel(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _parity(name, expect_small, tol=1e-10, **opts):
    _, args = load(name)
    F = G.native_form(**args)
    lp = BO.BoundedLP(F.A, F.b, F.c, F.u)
    with S.IpmSolver(F.A, F.b, F.c, ub=F.u, **opts) as sv:
        assert sv.m == F.A.shape[0] and sv.bounded == int(np.isfinite(F.u).sum())
        assert sv.schedule()["fused_small"] == expect_small
        sv.init_state(1.0)
        st = lp.start(1.0)
        # predictor at k = 0 (ipm_newton_direction) against the restatement; dy carries the conditioning of A Theta A^T
        # (KB2, GFRD-PNC: 2e-10 .. 3e-10 between two correct solves), dx and ds do not
        dx, dy, ds = sv.newton_direction(corrector=False)
        ox, oy, os_, _, _ = lp.predictor(*st)
        assert rel(dx, ox) < tol and rel(dy, oy) < 10 * tol and rel(ds, os_) < tol, (rel(dx, ox), rel(dy, oy), rel(ds, os_))
        sv.init_state(1.0)
        for k in range(3):
            sv.iterate(1)
            st = lp.iterate(*st)[:5]
            x, y, s = sv.get_state()
            w, z = sv.get_bound_state()
            for got, want, nm in zip((x, y, s, w, z), st, "xyswz"):
                if nm == "y":
                    # y itself carries the conditioning of A Theta A^T (GFRD-PNC: 1.8e-9 after two steps); A^T y, what the
                    # iteration uses, does not
                    assert rel(F.A.T @ np.ravel(got), F.A.T @ want) < tol and rel(got, want) < 100 * tol, (name, k + 1, nm, rel(got, want))
                else:
                    assert rel(got, want) < tol, (name, k + 1, nm, rel(got, want))
        return sv.schedule(), sv.factor


def test_parity_small_lp_kb2():
    sch, _ = _parity("KB2", 1)
    assert sch["fused_small"] == 1


def test_parity_dense_tile_grow22():
    sch, fac = _parity("GROW22", 0)
    assert fac == "dense" and sch["blocks"] == 4          # 440 rows: 4 blocks of 128 (1320 rows folded)


def test_parity_sparse_factor():
    # the multifrontal factor eliminates in its own (minimum-degree) order and this A Theta A^T is the least well conditioned
    # of the three: s drifts from the dense LAPACK factor of the restatement by 3e-10 after two steps, 1e-9 after three
    _, fac = _parity("GFRD-PNC", 0, tol=1e-8, factor="sparse")
    assert fac == "sparse"


def _known_optimum_lp(m, n, seed):
    """Dense LP with a known optimum built from complementary (x*, y*, s*, z*): a third of the bounded columns sit at 0,
    a third at u, a third inside; m interior columns in all (a square basis: x* and y* are unique, strictly complementary)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    u = np.full(n, np.inf)
    bnd = rng.permutation(n)[: n // 2]
    u[bnd] = rng.uniform(1.0, 3.0, bnd.size)
    x = np.zeros(n); s = np.zeros(n); z = np.zeros(n)
    perm = rng.permutation(n)
    interior = perm[:m]
    rest = perm[m:]
    x[interior] = np.where(np.isfinite(u[interior]), u[interior] * rng.uniform(0.2, 0.8, interior.size), rng.uniform(0.5, 2.0, interior.size))
    at_u = rest[np.isfinite(u[rest])][: max(1, rest.size // 4)]
    at_0 = np.setdiff1d(rest, at_u)
    x[at_u] = u[at_u]
    z[at_u] = rng.uniform(0.5, 2.0, at_u.size)
    s[at_0] = rng.uniform(0.5, 2.0, at_0.size)
    y = rng.standard_normal(m)
    b = A @ x
    c = A.T @ y + s - z
    return A, b, c, u, float(c @ x)


@pytest.mark.parametrize("m,n,fused,path", [(1024, 2048, "1", "plain"), (2048, 4096, "0", "overlapped"), (4096, 8192, "1", "fused")])
def test_dense_known_optimum(m, n, fused, path, monkeypatch):
    monkeypatch.setenv("IPM_FUSED_FACTOR", fused)
    A, b, c, u, opt = _known_optimum_lp(m, n, seed=m)
    with S.IpmSolver(A, b, c, ub=u, device=0) as sv:
        sv.init_state(0.0)
        st = sv.solve(tol=1e-9, tol_gap=1e-9 * max(1.0, abs(opt)), max_iter=200)      # gap bounds the objective error
        sch = sv.schedule()
        x, _, _ = sv.get_state()
        w, z = sv.get_bound_state()
    assert st["status"] == 1, (st["status"], st["iterations"], st["objective"], opt, st["rp_norm"], st["rd_norm"], st["gap"])
    assert abs(st["objective"] - opt) <= 1e-8 * max(1.0, abs(opt))
    x = x.ravel()
    U = np.isfinite(u)
    assert np.all(x >= 0) and np.all(x[U] <= u[U] * (1 + 1e-8) + 1e-8)
    assert np.all(w.ravel()[~U] == 0) and np.all(z.ravel()[~U] == 0)
    if path == "fused":
        assert sch["fused_factor"] == 1
    else:
        assert sch["fused_factor"] == 0
    assert sch["blocks"] == m // 128


def _folded_mehrotra_ok():
    """Bounded general-form files the folded Mehrotra path solves within 1e-5 of the Netlib optimum."""
    return ["80BAU3B", "BOEING1", "BOEING2", "BORE3D", "CZPROB", "ETAMACRO", "FIT1P", "FORPLAN", "GANGES", "GFRD-PNC",
            "GROW15", "GROW22", "GROW7", "KB2", "MAROS", "NESM", "PILOT87", "PILOTNOV", "SEBA", "SHELL", "SIERRA",
            "STANDATA", "STANDMPS"]


@pytest.mark.parametrize("name", _folded_mehrotra_ok())
def test_native_converges_general_form(name):
    z, args = load(name)
    obj, info = G.new_interior_sparse(**args, tol=1e-8, bounds="native", start="mehrotra", return_info=True)
    o = float(z["netlib_optimum"])
    assert info["status"] == 1, (name, info["status_name"], info["iterations"])
    assert abs(obj - o) <= 1e-5 * max(1.0, abs(o)), (name, obj, o)
    lb, ub = np.ravel(args["lb"]), np.ravel(args["ub"])
    assert info["fixed_removed"] == int((lb == ub).sum())
    assert info["bounded"] == int((np.isfinite(ub) & (lb != ub)).sum())     # CZPROB, MAROS: every finite bound is a fixed variable


@pytest.mark.parametrize("name", ["PILOT87", "NESM"])
def test_normal_matrix_order_is_m(name):
    z, args = load(name)
    F = G.native_form(**args)
    m = int(z["std0_A_shape"][0])
    with S.IpmSolver(F.A, F.b, F.c, ub=F.u) as sv:
        assert sv.m == m
        if sv.factor == "dense":
            assert sv.schedule()["blocks"] == (m + 127) // 128
        assert sv.m < int(z["std_A_shape"][0])


def test_restart_restores_bound_state_qap8():
    A, b, c, cTlb = load_netlib("QAP8")
    u = np.ones(A.shape[1])                        # implied by the assignment constraints: the optimum stays 203.5
    x, y, s, info = S.solve_with_info(A, b, c, tol=1e-8, ub=u, y0=1.0, max_iter=500)
    assert info["auto_regularized"] == 1 and info["status"] == 1
    assert abs(info["objective"] - cTlb - 203.5) <= 1e-6 * 203.5
    assert info["bounded"] == A.shape[1]


def _traj(A, b, c, **kw):
    x, y, s, info = S.solve_with_info(A, b, c, tol=1e-8, history=True, **kw)
    return np.concatenate([x.ravel(), y.ravel(), s.ravel()]), info


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_infinite_ub_is_bit_identical(kind):
    from oracle import ipm_oracle as O
    if kind == "dense":
        A, b, c = O.synthetic_lp(300, 700, seed=5)
        kw = dict(y0=0.0)
    else:
        A, b, c, _ = load_netlib("BANDM")
        kw = dict(y0=1.0)
    v0, i0 = _traj(A, b, c, **kw)
    v1, i1 = _traj(A, b, c, ub=np.full(A.shape[1], np.inf), **kw)
    assert i1["bounded"] == 0 and "w" not in i1
    assert np.array_equal(v0, v1)
    assert i0["history"] == i1["history"] and i0["objective"] == i1["objective"]


def test_native_on_unbounded_file_is_bit_identical():
    _, args = load("AFIRO")
    o0, i0 = G.new_interior_sparse(**args, tol=1e-8, return_info=True)
    o1, i1 = G.new_interior_sparse(**args, tol=1e-8, return_info=True, bounds="native")
    assert o0 == o1 and i0["iterations"] == i1["iterations"] and i1["bounded"] == 0


def test_bounded_solve_is_bitwise_repeatable():
    _, args = load("GROW22")
    F = G.native_form(**args)
    out = []
    for _ in range(2):
        x, y, s, info = S.solve_with_info(F.A, F.b, F.c, ub=F.u, tol=1e-8, tol_gap=1e-6, start="mehrotra", history=True)
        out.append((np.concatenate([x.ravel(), y.ravel(), s.ravel(), info["w"].ravel(), info["z"].ravel()]), info["history"]))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


def test_lockstep_refuses_bounded_solver():
    _, args = load("GROW22")
    F = G.native_form(**args)
    with S.IpmSolver(F.A, F.b, F.c, ub=F.u, lockstep=True, concurrent=True) as sv:
        sv.init_state(1.0)
        assert not S.lockstep_eligible(sv)
        with S.LockstepBatch() as batch:
            with pytest.raises(_lib.IpmError):
                batch.add(sv)
        with pytest.raises(_lib.IpmError):
            S.solve_lockstep([sv])
