"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against NumPy, the oracle
and the golden vectors generated from the reference.  fp64 throughout; the north-star
tolerance is 1e-6 relative on objective and scaled residuals, kernel-level
comparisons use much tighter bounds written next to each assert."""
import os

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

import interiorpointmethod_amd as ipm                      # noqa: E402
from interiorpointmethod_amd.matio import load_npz_problem  # noqa: E402
from interiorpointmethod_amd.workloads import synthetic_lp  # noqa: E402
from oracle import ipm_oracle as O                          # noqa: E402


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("m,n", [(1, 1), (16, 32), (127, 65), (128, 64), (129, 1000), (200, 300), (1000, 2000)])
def test_form_normal_matrix(m, n):
    rng = np.random.default_rng(m * 7 + n)
    A = rng.standard_normal((m, n))
    d = rng.uniform(1e-3, 1e3, n)
    with ipm.IpmSolver(A, np.zeros(m), np.zeros(n)) as sv:
        B = sv.form_normal_matrix(d)
    ref = (A * d) @ A.T
    assert rel(B, ref) < 1e-13
    assert np.array_equal(B, B.T)


def test_form_exact_integers_asymmetric():
    """Exact small-integer data: any wrong MFMA lane map or tile offset shows as a nonzero diff."""
    m, n = 150, 70
    A = (np.arange(m * n).reshape(m, n) * 7 % 11 - 5).astype(np.float64)
    A[3, 5] = 13.0
    d = (np.arange(n) % 5 + 1).astype(np.float64)
    with ipm.IpmSolver(A, np.zeros(m), np.zeros(n)) as sv:
        B = sv.form_normal_matrix(d)
    assert np.array_equal(B, (A * d) @ A.T)


def test_form_wide_dynamic_range():
    """d spans > 50 decades on the reference's trajectories."""
    rng = np.random.default_rng(5)
    m, n = 90, 400
    A = rng.standard_normal((m, n))
    d = 10.0 ** rng.uniform(-40, 15, n)
    with ipm.IpmSolver(A, np.zeros(m), np.zeros(n)) as sv:
        B = sv.form_normal_matrix(d)
    ref = (A * d) @ A.T
    assert rel(B, ref) < 1e-12


@pytest.mark.parametrize("m", [1, 16, 100, 128, 129, 300, 700, 1500, 2048, 3000])   # >= 2048: grouped-inverse solves
def test_cholesky_and_solve(m):
    rng = np.random.default_rng(m)
    M = rng.standard_normal((m, m + 10))
    B = M @ M.T + 0.1 * np.eye(m)
    rhs = rng.standard_normal(m)
    with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
        z, nfix = sv.solve_linear(B, rhs)
        L = sv.get_factor()
    assert nfix == 0
    assert rel(L, np.linalg.cholesky(B)) < 1e-11
    assert np.linalg.norm(B @ z.ravel() - rhs) / np.linalg.norm(rhs) < 1e-10


def test_solve_linear_is_linear_and_deterministic():
    rng = np.random.default_rng(11)
    m = 400
    M = rng.standard_normal((m, m))
    B = M @ M.T + np.eye(m)
    r1, r2 = rng.standard_normal(m), rng.standard_normal(m)
    with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
        z1, _ = sv.solve_linear(B, r1)
        z2, _ = sv.solve_linear(B, r2)
        z12, _ = sv.solve_linear(B, 2.0 * r1 - 3.0 * r2)
        z1b, _ = sv.solve_linear(B, r1)
    assert rel(z12, 2.0 * z1 - 3.0 * z2) < 1e-10
    assert np.array_equal(z1, z1b)                       # fixed-order reductions: bitwise reproducible


def test_pivot_guard_rank_deficient():
    """rank-deficient normal matrices must not produce NaN; the guard reports its fixes."""
    rng = np.random.default_rng(7)
    m = 200
    M = rng.standard_normal((m, 150))
    B = M @ M.T
    rhs = B @ rng.standard_normal(m)
    with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
        z, nfix = sv.solve_linear(B, rhs)
    assert 40 <= nfix <= 60 and np.all(np.isfinite(z))
    assert np.linalg.norm(B @ z.ravel() - rhs) / np.linalg.norm(rhs) < 1e-6
    Lo, fo = O.guarded_cholesky(B)
    assert abs(fo - nfix) <= 5


def test_tiny_normal_matrix_is_not_guarded():
    """max diag(B) over the true rows sets the guard scale: a uniformly tiny B (d ~ 1e-41 on the
    AFIRO trajectory) must factor without a single fix."""
    rng = np.random.default_rng(2)
    m = 27
    M = rng.standard_normal((m, 60))
    B = (M @ M.T) * 1e-41
    rhs = rng.standard_normal(m)
    with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
        z, nfix = sv.solve_linear(B, rhs)
    assert nfix == 0
    assert np.linalg.norm(B @ z.ravel() - rhs) / np.linalg.norm(rhs) < 1e-9


# ------------------------------------------------------------------ sparse-A front end
@pytest.mark.parametrize("m,n,dens", [(5, 9, 0.5), (130, 400, 0.02), (700, 1500, 0.004), (300, 200, 0.05)])
def test_sparse_formation_matches_dense(m, n, dens):
    """The sparse formation of B (sparse_ops.h) against the dense MFMA path on the same matrix, including an
    empty row and an empty column.  (The SpMVs: tests/test_gpu_sparse_front.py.)"""
    rng = np.random.default_rng(m + n)
    A = sparse.random(m, n, density=dens, random_state=np.random.RandomState(m), format="lil")
    A[0, :] = 0.0
    A[:, n - 1] = 0.0
    A[m - 1, 0] = 2.5
    A = sparse.csc_matrix(A)
    d = 10.0 ** rng.uniform(-6, 6, n)
    with ipm.IpmSolver(A, np.zeros(m), np.zeros(n)) as sp_, ipm.IpmSolver(A, np.zeros(m), np.zeros(n), dense=True) as de_:
        assert sp_.sparse and not de_.sparse
        Bs, Bd = sp_.form_normal_matrix(d), de_.form_normal_matrix(d)
    ref = (A @ sparse.diags(d) @ A.T).toarray()
    assert rel(Bs, ref) < 1e-13 and rel(Bd, ref) < 1e-13
    assert np.array_equal(Bs, Bs.T)


@pytest.mark.parametrize("name", ["AFIRO", "BANDM", "SCSD6"])
def test_sparse_and_dense_paths_agree(golden_dir, name):
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    with ipm.IpmSolver(A, b, c) as sp_, ipm.IpmSolver(A, b, c, dense=True) as de_:
        sp_.init_state(1.0); de_.init_state(1.0)
        d1 = sp_.newton_direction(False); d2 = de_.newton_direction(False)
        for u, v in zip(d1, d2):
            assert rel(u, v) < 1e-9
        st1 = sp_.solve(tol=1e-8, max_iter=500)
        sp_.init_state(1.0)
        st1b = sp_.solve(tol=1e-8, max_iter=500)
        de_.init_state(1.0)
        st2 = de_.solve(tol=1e-8, max_iter=500)
    assert st1["status"] == 1 and st2["status"] == 1
    assert abs(st1["objective"] - st2["objective"]) <= 1e-8 * max(1.0, abs(st2["objective"]))
    assert st1["objective"] == st1b["objective"] and st1["iterations"] == st1b["iterations"]   # reproducible


@pytest.mark.parametrize("name", ["SC205", "BANDM", "DEGEN2"])
def test_list_formation_bit_identical(golden_dir, monkeypatch, name):
    """Sparse handles with 128 < m and <= 1536 padded rows form B from the host-built product list (adat_list_kernel, one
    thread per entry); it performs the same products in the same order as the row-owner kernel (adat_sparse_kernel,
    IPM_LIST_FORM=0), so B, the factor and the whole solve are bit-identical between the two."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    rng = np.random.default_rng(3)
    d = 10.0 ** rng.uniform(-8, 8, A.shape[1])
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("IPM_LIST_FORM", flag)
        with ipm.IpmSolver(A, b, c) as sv:
            B = sv.form_normal_matrix(d)
            sv.init_state(1.0)
            st = sv.solve(tol=1e-8, max_iter=300)
            out[flag] = (B, sv.get_factor(), sv.get_state(), st)
    assert np.array_equal(out["1"][0], out["0"][0]) and np.array_equal(out["1"][1], out["0"][1])
    assert out["1"][3]["iterations"] == out["0"][3]["iterations"] and out["1"][3]["status"] == 1
    for u, v in zip(out["1"][2], out["0"][2]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("name", ["SC50A", "BANDM", "SCSD6"])
def test_reordered_rows_same_seam(golden_dir, name):
    """reorder="rcm" permutes the rows of A on the device (smaller tile envelope of A A^T); the seam must not
    notice: B, directions (dy un-permuted), iterates and the solve agree with the natural order."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    rng = np.random.default_rng(5)
    d = 10.0 ** rng.uniform(-3, 3, A.shape[1])
    with ipm.IpmSolver(A, b, c, reorder=None) as nat, ipm.IpmSolver(A, b, c, reorder="rcm") as rcm:
        assert nat._perm is None and sorted(rcm._perm.tolist()) == list(range(A.shape[0]))
        assert rel(rcm.form_normal_matrix(d), nat.form_normal_matrix(d)) < 1e-13
        nat.init_state(1.0); rcm.init_state(1.0)
        for u, v in zip(rcm.newton_direction(False), nat.newton_direction(False)):
            assert rel(u, v) < 1e-9
        y0 = rng.standard_normal(A.shape[0])
        x0 = rng.uniform(0.5, 2, A.shape[1]); s0 = rng.uniform(0.5, 2, A.shape[1])
        nat.set_state(x0, y0, s0); rcm.set_state(x0, y0, s0)
        assert np.array_equal(rcm.get_state()[1].ravel(), y0)              # round trip through the permutation
        nat.iterate(1); rcm.iterate(1)
        for u, v in zip(rcm.get_state(), nat.get_state()):
            assert rel(u, v) < 1e-9
        nat.init_state(1.0); rcm.init_state(1.0)
        s1, s2 = rcm.solve(tol=1e-8, max_iter=500), nat.solve(tol=1e-8, max_iter=500)
    assert s1["status"] == 1 and s2["status"] == 1
    assert abs(s1["objective"] - s2["objective"]) <= 1e-8 * max(1.0, abs(s2["objective"]))


def test_tile_envelope_skips_only_zeros():
    """Block-bidiagonal A (staircase LP, 2500 rows): A A^T is block tridiagonal, so its tile envelope is 2-3 blocks of
    20 and the factorization / triangular solves skip the rest.  The direction must equal the dense path's (which
    skips nothing) and IPM_ENVELOPE=0 on the same handle type."""
    rng = np.random.default_rng(11)
    nbk, bs, cs = 25, 100, 160
    blocks = [[None] * nbk for _ in range(nbk)]
    for i in range(nbk):
        blocks[i][i] = sparse.random(bs, cs, density=0.05, random_state=np.random.RandomState(i), format="csr") + \
            sparse.eye(bs, cs, format="csr")
        if i + 1 < nbk:
            blocks[i + 1][i] = sparse.random(bs, cs, density=0.02, random_state=np.random.RandomState(100 + i), format="csr")
    A = sparse.csc_matrix(sparse.bmat(blocks))
    m, n = A.shape
    x0 = rng.uniform(0.5, 1.5, n); y0 = rng.standard_normal(m); s0 = rng.uniform(0.5, 1.5, n)
    b, c = A @ x0, A.T @ y0 + s0
    with ipm.IpmSolver(A, b, c, reorder=None) as sp_, ipm.IpmSolver(A, b, c, dense=True) as de_:
        assert sp_.sparse and sp_.factor == "dense" and sp_.schedule()["envelope"] == 1
        sp_.init_state(1.0); de_.init_state(1.0)
        for u, v in zip(sp_.newton_direction(False), de_.newton_direction(False)):
            assert rel(u, v) < 1e-10
        L1, L2 = sp_.get_factor(), de_.get_factor()
        assert rel(L1, L2) < 1e-10
        assert np.count_nonzero(L1[1000:, :300]) == 0                       # far below the envelope: never touched
        st1, st2 = sp_.solve(tol=1e-8, max_iter=200), de_.solve(tol=1e-8, max_iter=200)
    assert st1["status"] == 1 and st1["iterations"] == st2["iterations"]
    assert abs(st1["objective"] - st2["objective"]) <= 1e-9 * max(1.0, abs(st2["objective"]))


# ------------------------------------------------------------------ direction seam vs the reference
@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "BANDM"])
def test_direction_kats(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "kat_%s.npz" % name))
    m, n = (int(v) for v in z["shape"])
    A = sparse.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(m, n))
    with ipm.IpmSolver(A, z["b"], z["c"]) as sv:
        k = 0                                            # start point: well conditioned, tight bound
        pre = "k0_"
        sv.set_state(z[pre + "x"], z[pre + "y"], z[pre + "s"])
        dxa, dya, dsa = sv.newton_direction(False)
        st = dict(sv.stats)
        assert rel(dxa, z[pre + "dxa"]) < 1e-11 and rel(dya, z[pre + "dya"]) < 1e-11 and rel(dsa, z[pre + "dsa"]) < 1e-11
        assert rel(dxa, z[pre + "normal_dxa"]) < 1e-11          # reference method="normal", main.py:221-229
        assert np.isclose(st["alpha_aff_p"], float(z[pre + "alpha_aff_p"]), rtol=1e-10)
        assert np.isclose(st["alpha_aff_d"], float(z[pre + "alpha_aff_d"]), rtol=1e-10)
        dx, dy, ds = sv.newton_direction(True)
        assert np.isclose(sv.stats["sigma"], float(z[pre + "sigma"]), rtol=1e-9)
        assert np.isclose(sv.stats["mu"], float(z[pre + "mu"]), rtol=1e-12)
        assert rel(dx, z[pre + "dx"]) < 1e-10 and rel(dy, z[pre + "dy"]) < 1e-10 and rel(ds, z[pre + "ds"]) < 1e-10
        # one full iteration reproduces the reference's next iterate
        sv.set_state(z[pre + "x"], z[pre + "y"], z[pre + "s"])
        st = sv.iterate(1)
        xn, yn, sn = sv.get_state()
        assert np.isclose(st["alpha_p"], float(z[pre + "alpha_p"]), rtol=1e-9)
        assert np.isclose(st["alpha_d"], float(z[pre + "alpha_d"]), rtol=1e-9)
        assert rel(xn, z[pre + "xn"]) < 1e-10 and rel(yn, z[pre + "yn"]) < 1e-10 and rel(sn, z[pre + "sn"]) < 1e-10
        # a later iterate (ill-conditioned: dy/ds still agree with the full-KKT reference)
        k = int(z["iters"][1])
        pre = "k%d_" % k
        sv.set_state(z[pre + "x"], z[pre + "y"], z[pre + "s"])
        dxa, dya, dsa = sv.newton_direction(False)
        assert rel(dya, z[pre + "dya"]) < 1e-8 and rel(dsa, z[pre + "dsa"]) < 1e-8 and rel(dxa, z[pre + "dxa"]) < 1e-8
        # the last stored iterate (d = x/s spans up to 1e22): the reference's OWN two formulations (method="full" LU
        # and method="normal") no longer agree with each other there -- AFIRO k=60: 96 % apart in dxa, BANDM k=30:
        # 4e-6 in dya -- so each component is compared with the reference's method="normal" output (the formulation
        # the device implements) with a bound tied to that disagreement, and skipped where it exceeds 1e-3.
        k = int(z["iters"][2])
        pre = "k%d_" % k
        sv.set_state(z[pre + "x"], z[pre + "y"], z[pre + "s"])
        got = sv.newton_direction(False)
        for g, nm in zip(got, ("dxa", "dya", "dsa")):
            spread = rel(z[pre + "normal_" + nm], z[pre + nm])
            if spread < 1e-3:
                assert rel(g, z[pre + "normal_" + nm]) < max(1e-8, 100.0 * spread), (name, k, nm, spread)


def test_qap15_direction_kat(golden_dir):
    """Config 3 (QAP15, 6330 x 22275, rank-deficient): predictor direction at the start point vs the
    reference's method="normal" (18 s of SuperLU there).  A is rank deficient, so dy is not unique;
    A^T dy, dx and ds are, and those are compared."""
    z = np.load(os.path.join(golden_dir, "kat_QAP15_normal_k0.npz"))
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "QAP15.npz"))
    m, n = A.shape
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(1.0)
        dxa, dya, dsa = sv.newton_direction(False)
        st = dict(sv.stats)
    assert rel(dxa, z["dxa"]) < 1e-6 and rel(dsa, z["dsa"]) < 1e-6
    assert np.isclose(st["alpha_aff_p"], float(z["alpha_aff_p"]), rtol=1e-6)
    assert np.isclose(st["alpha_aff_d"], float(z["alpha_aff_d"]), rtol=1e-6)


# ------------------------------------------------------------------ solver seam vs the reference
@pytest.mark.parametrize("nm", ["ex1", "ex2", "ex3", "syn_64x128", "syn_256x512", "syn_512x1024", "syn_1024x2048"])
def test_dense_end_to_end(golden_dir, nm):
    z = np.load(os.path.join(golden_dir, "dense_%s.npz" % nm))
    if nm.startswith("syn"):
        m, n = (int(v) for v in z["shape"])
        A, _, _ = synthetic_lp(m, n)
        b, c = z["b"], z["c"]          # exactly the LP the reference solved (a threaded matvec differs in the last bits)
    else:
        A, b, c = z["A"], z["b"], z["c"]
    x, y, s, info = ipm.solve_with_info(A, b, c, tol=1e-8, y0=0.0, max_iter=50000)
    ref = float(z["objective"])
    assert info["status_name"] == "converged"
    assert abs(info["objective"] - ref) <= 1e-6 * max(1.0, abs(ref))
    assert info["rp"] <= 1e-6 and info["rd"] <= 1e-6 and info["gap"] <= 1e-8
    assert abs(info["iterations"] - int(z["iterations"])) <= 2
    if nm.startswith("syn"):                       # ex2's optimal face is not a single point
        assert rel(x, z["x"]) < 1e-5
    assert x.shape == (A.shape[1], 1) and y.shape == (A.shape[0], 1) and s.shape == x.shape


PARITY_FAST = ["AFIRO", "BANDM", "DEGEN2", "E226", "FIT1P", "GROW15", "GROW22", "GROW7", "KB2", "SC105", "SC205",
               "SC50A", "SC50B", "SCSD1", "SCSD6", "SCSD8", "SCTAP1", "SCTAP2", "SCTAP3", "SHARE2B", "STOCFOR1",
               "STOCFOR2", "STOCFOR3", "TRUSS", "WOODW", "MAROS-R7"]


@pytest.mark.parametrize("name", PARITY_FAST)
def test_netlib_parity(golden_dir, name):
    """Parity set of BASELINE.md 2.4 (the files on which the verbatim reference loop converges)."""
    e = np.load(os.path.join(golden_dir, "e2e_%s.npz" % name))
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    x, y, s, info = ipm.solve_with_info(A, b, c, tol=1e-8, y0=1.0, max_iter=5000)
    ref = float(e["objective"])
    assert info["status_name"] == "converged", info
    assert abs(info["objective"] - ref) <= 1e-6 * max(1.0, abs(ref))
    assert info["rp"] <= 1e-6 and info["rd"] <= 1e-6 and info["gap"] <= 1e-8
    if name != "DEGEN2":      # guarded Cholesky legitimately converges in ~24 instead of 223
        assert abs(info["iterations"] - int(e["iterations"])) <= 2
    # the returned iterate satisfies the reference's own stop test on the host
    assert not O.check_optimality(*O.as_float64_problem(A, b, c), x, y, s, 1e-8, 1e-8, 1e-8)


def test_qap15_config3_objective(golden_dir):
    """BASELINE.json configs[2]: QAP15 (6330 x 22275, rank deficient) through the PLAIN call solve(A, b, c).  A
    verbatim reference solve is intractable (one normal-equations step = 18 s of SuperLU), so the pin is
    the Netlib optimum 1.0409940410e3 (main.py:1474, benchmarks/readme.txt:141) to 1e-6 relative.  The guard alone
    stalls on the QAP family: the first factorization guards > 5 % of its pivots, the library switches
    the 1e-14 Tikhonov shift on and restarts the solve (ipm_stats.auto_regularized)."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "QAP15.npz"))
    x, y, s, info = ipm.solve_with_info(A, b, c, tol=1e-8, y0=1.0, max_iter=300)
    assert info["auto_regularized"] == 1
    assert info["status_name"] == "converged" and info["iterations"] < 60
    assert abs(info["objective"] - 1.0409940410e3) <= 1e-6 * 1.0409940410e3
    assert info["rp"] <= 1e-6 and info["rd"] <= 1e-6 and info["gap"] <= 1e-8
    Af, bf, cf = O.as_float64_problem(A, b, c)
    assert np.linalg.norm(Af @ x - bf) / (1 + np.linalg.norm(bf)) <= 1e-6      # host-side re-check
    assert np.all(x > 0) and np.all(s > 0)


@pytest.mark.parametrize("name,ref", [("QAP8", 2.0350000000e2), ("QAP12", 5.2289435056e2)])
def test_qap_family_default_call(golden_dir, name, ref):
    """Plain solve(A, b, c) on the rest of the QAP family; the explicit option gives the same answer bit for bit
    (the restart begins from the same start state with the same shift); with the automatic switch off the guard-only
    loop of QAP12 runs into the iteration cap (the round-1 behaviour)."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    x, y, s, info = ipm.solve_with_info(A, b, c, tol=1e-8, y0=1.0, max_iter=300)
    assert info["auto_regularized"] == 1
    assert info["status_name"] == "converged" and abs(info["objective"] - ref) <= 1e-6 * ref      # readme.txt:139-140
    x2, _, _, info2 = ipm.solve_with_info(A, b, c, tol=1e-8, y0=1.0, max_iter=300, regularize=1e-14)
    assert info2["auto_regularized"] == 0 and info2["iterations"] == info["iterations"] and np.array_equal(x, x2)
    if name == "QAP12":
        _, _, _, off = ipm.solve_with_info(A, b, c, tol=1e-8, y0=1.0, max_iter=300, auto_regularize=False)
        assert off["auto_regularized"] == 0 and off["status"] == 2          # guard only: runs into the cap


@pytest.mark.parametrize("name", ["AFIRO", "DEGEN2", "STOCFOR1", "SCTAP1", "BANDM"])
def test_auto_regularize_leaves_parity_lps_untouched(golden_dir, name):
    """The automatic switch must not change anything outside the QAP family: DEGEN2 (2 dependent rows of 444), STOCFOR1
    and SCTAP1 (guarded pivots late in the solve) and two full-rank files give bit-identical iterates with the switch
    on (default) and off."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    x1, y1, s1, i1 = ipm.solve_with_info(A, b, c, tol=1e-8, max_iter=5000)
    x2, y2, s2, i2 = ipm.solve_with_info(A, b, c, tol=1e-8, max_iter=5000, auto_regularize=False)
    assert i1["auto_regularized"] == 0 and i1["iterations"] == i2["iterations"] and i1["status"] == 1
    assert np.array_equal(x1, x2) and np.array_equal(y1, y2) and np.array_equal(s1, s2)


def test_interior_sparse_drop_in(golden_dir):
    """interior_sparse(A, b, c, cTlb, tol) returns sum(x*c) - cTlb like main.py:815."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "AFIRO.npz"))
    obj = ipm.interior_sparse(A, b, c, cTlb, tol=1e-8)
    assert abs(obj - (-464.7531428559395)) < 1e-6 * 464.75
    assert abs(obj - (-4.6475314286e2)) < 1e-5            # Netlib optimum, benchmarks/readme.txt:88
    assert ipm.last_info()["iterations"] in (92, 93, 94, 95)


def test_reference_named_entry_points(golden_dir):
    """The host mirror keeps the reference's names and argument meaning (SURVEY 8b seams 1-3)."""
    z = np.load(os.path.join(golden_dir, "dense_ex3.npz"))
    obj = ipm.interior(z["A"], z["b"], z["c"], tol=1e-8)                     # main.py:707 (y0 = 0, cap 50000)
    assert abs(obj - float(z["objective"])) <= 1e-6 * abs(float(z["objective"]))
    k = np.load(os.path.join(golden_dir, "kat_SC50A.npz"))
    m, n = (int(v) for v in k["shape"])
    A = sparse.csc_matrix((k["A_data"], k["A_indices"], k["A_indptr"]), shape=(m, n))
    x, y, s = k["k0_x"], k["k0_y"], k["k0_s"]
    dx, dy, ds = ipm.direction_predicted_sparse(A, k["b"], k["c"], x, y, s, method="normal")   # main.py:197
    assert rel(dx, k["k0_normal_dxa"]) < 1e-10 and rel(dy, k["k0_normal_dya"]) < 1e-10
    dx, dy, ds = ipm.direction_corrected_sparse(A, k["b"], k["c"], x, y, s, dx, dy, ds)         # main.py:247
    assert rel(dx, k["k0_dx"]) < 1e-9 and rel(ds, k["k0_ds"]) < 1e-9
    dxf, dyf, dsf = ipm.direction_predicted_sparse(A, k["b"], k["c"], x, y, s, method="full")    # main.py:198-212
    assert rel(dxf, k["k0_dxa"]) < 1e-10 and rel(dyf, k["k0_dya"]) < 1e-10 and rel(dsf, k["k0_dsa"]) < 1e-10
    with pytest.raises(ValueError):
        ipm.direction_predicted_sparse(A, k["b"], k["c"], x, y, s, method="eliminate")
    e1 = np.load(os.path.join(golden_dir, "dense_ex1.npz"))                  # dense-path names, main.py:185-244
    n1 = e1["A"].shape[1]
    da = ipm.direction_predicted(e1["A"], e1["b"], e1["c"], np.ones(n1), np.zeros(e1["A"].shape[0]), np.ones(n1))
    assert rel(da[0], e1["k0_dxa"]) < 1e-11 and rel(da[1], e1["k0_dya"]) < 1e-11 and rel(da[2], e1["k0_dsa"]) < 1e-11
    dc = ipm.direction_corrected(e1["A"], e1["b"], e1["c"], np.ones(n1), np.zeros(e1["A"].shape[0]), np.ones(n1), *da)
    assert rel(dc[0], e1["k0_dx"]) < 1e-10 and rel(dc[1], e1["k0_dy"]) < 1e-10 and rel(dc[2], e1["k0_ds"]) < 1e-10
    rng = np.random.default_rng(1)
    M = rng.standard_normal((90, 120))
    B = M @ M.T
    rhs = rng.standard_normal((90, 1))
    zz = ipm.solve_linear(B, rhs)                                                # main.py:176
    assert zz.shape == (90, 1) and np.linalg.norm(B @ zz - rhs) / np.linalg.norm(rhs) < 1e-10


def test_integer_dtype_inputs(golden_dir):
    """the .mat files hold int16/uint8 arrays; the boundary casts to float64."""
    A, b, c = np.array([[3, 6, 8], [8, 4, 1]], dtype=np.int16), np.array([30, 44], dtype=np.uint8), \
        np.array([-100, -125, -20], dtype=np.int16)
    x, y, s = ipm.solve(A, b, c, tol=1e-8, y0=0.0)
    assert abs(float(c @ x.ravel()) + 775) < 1e-5           # ex1 optimum, main.py:1253


def test_invalid_inputs_rejected(golden_dir):
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "CAPRI.npz"))
    assert not valid
    with pytest.raises(ipm.IpmError) as ei:
        ipm.solve(A, b, c)
    assert ei.value.code == -6


# ------------------------------------------------------------------ BASELINE.json full size
def test_dense_4096x8192_full_solve(golden_dir):
    """configs[1] against the REFERENCE ITSELF: tests/golden/dense_syn_4096x8192.npz holds the verbatim dense solve of
    this LP by the reference's own step functions (main.py:185-244, 604-697; two LAPACK gesv of a 20480^2 KKT matrix
    per iteration, 40 minutes in the build container): 24 iterations, objective -3.7612544745317e+02, the final
    (x, y, s), the objective after every iteration and the first step's scalars."""
    z = np.load(os.path.join(golden_dir, "dense_syn_4096x8192.npz"))
    A, _, _ = synthetic_lp(4096, 8192)
    b, c = z["b"], z["c"]                 # the LP the reference solved (threaded matvec: last bits differ per host)
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        da = sv.newton_direction(False)                       # reference: direction_predicted (full KKT, LAPACK gesv)
        dc = sv.newton_direction(True)                        # reference: direction_corrected
        for g, nm in zip(da + dc, ("dxa", "dya", "dsa", "dx", "dy", "ds")):
            assert rel(g, z["k0_" + nm]) < 1e-9, nm
        sv.init_state(0.0)
        first = sv.iterate(1)
        xn, yn, sn = sv.get_state()
        assert rel(xn, z["k0_xn"]) < 1e-10 and rel(yn, z["k0_yn"]) < 1e-10 and rel(sn, z["k0_sn"]) < 1e-10
        sv.init_state(0.0)
        st = sv.solve(tol=1e-8, max_iter=200)
        x, y, s = sv.get_state()
        hist = sv.history()
        sv.init_state(0.0)
        st2 = sv.solve(tol=1e-8, max_iter=200)
        x2, _, _ = sv.get_state()
    # first step: the reference's ratio tests, centering and damped step lengths (main.py:305-322, 588-626)
    assert np.isclose(first["alpha_aff_p"], float(z["k0_alpha_aff_p"]), rtol=1e-9)
    assert np.isclose(first["alpha_aff_d"], float(z["k0_alpha_aff_d"]), rtol=1e-9)
    assert np.isclose(first["sigma"], float(z["k0_sigma"]), rtol=1e-8)
    assert np.isclose(first["alpha_p"], float(z["k0_alpha_p"]), rtol=1e-9) and np.isclose(first["alpha_d"], float(z["k0_alpha_d"]), rtol=1e-9)
    # whole solve: iteration count, objective, iterate, and the objective trajectory
    ref = float(z["objective"])
    assert st["status"] == 1 and st["iterations"] == int(z["iterations"]) == 24
    assert abs(st["objective"] - ref) <= 1e-9 * abs(ref)
    assert rel(x, z["x"]) < 1e-6 and rel(s, z["s"]) < 1e-6 and rel(y, z["y"]) < 1e-6
    traj = np.array([r["objective"] for r in hist[1:]] + [st["objective"]])        # objective after iteration 1..24
    assert np.allclose(traj, z["objective_after_iteration"], rtol=1e-8, atol=1e-8)
    # size-independent properties: feasibility, complementarity, weak duality gap closes
    rb = A @ x - b
    rc = A.T @ y + s - c
    assert np.linalg.norm(rb) / (1 + np.linalg.norm(b)) < 1e-8
    assert np.linalg.norm(rc) / (1 + np.linalg.norm(c)) < 1e-8
    assert np.all(x > 0) and np.all(s > 0) and (x.T @ s).item() <= 1e-8
    assert abs((c.T @ x).item() - (b.T @ y).item()) <= 1e-6 * 3.77e2
    assert np.array_equal(x, x2) and st2["iterations"] == st["iterations"]     # bitwise reproducible


# General-form LPs of the reference's benchmarks_full set on which the HIP path converges (tools/general_report.py over
# all 39 fixtures).  The reference's own driver reaches the optimum on the first 12; on KB2 and SCORPION it never passes
# its stop test (returns 18.49 / 0.0) and on STANDATA it silently drops the nonzero lower bounds (returns 847.8):
# there the pin is the Netlib optimum alone.  ADLITTLE is in the conversion fixtures only: the reference runs it to its
# 999-iteration cap (dual residual stalls at 1.5e-3) and just happens to return the optimum from there.
# STANDATA left this list in round 2: from the reference's start x = s = y = 1 it needed a 190-iteration chaotic trajectory
#  that a change of summation order in the triangular solves no longer reproduces (the loop now ends in NaN
# after 673 iterations, like the reference's own loop does on 25 of the 81 standard-form files).  It is solved, with the
# other 39 small general-form files, from the Mehrotra start (test_general_form_all_fixtures_with_mehrotra_start).
GENERAL = ["AFIRO", "BANDM", "DEGEN2", "E226", "SC105", "SC205", "SC50A", "SC50B", "SCSD1", "SCTAP1", "SHARE2B", "STOCFOR1",
           "KB2", "SCORPION"]


@pytest.mark.parametrize("name", GENERAL)
def test_new_interior_sparse_general_form(golden_dir, name):
    """The general-form driver (main.py:1081-1245) on the reference's benchmarks_full inputs: objective within 1e-6
    relative of the Netlib optimum, and of what the reference's own new_interior_sparse returns (tol=1e-8, e3=1e-6)
    wherever that run reached the optimum."""
    from interiorpointmethod_amd import general_form as G
    z = np.load(os.path.join(golden_dir, "general", name + ".npz"))

    def mat(prefix):
        if prefix + "_none" in z.files:
            return None
        return sparse.csc_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]),
                                 shape=tuple(int(v) for v in z[prefix + "_shape"]))
    obj, info = G.new_interior_sparse(c=z["c"], Aineq=mat("Aineq"), bineq=z["bineq"] if "bineq" in z.files else None,
                                      Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, lb=z["lb"], ub=z["ub"],
                                      tol=1e-8, return_info=True)
    opt, ref = float(z["netlib_optimum"]), float(z["ref_objective"])
    assert info["status"] == 1 and info["iterations"] <= 999
    assert abs(obj - opt) <= 1e-6 * max(1.0, abs(opt))
    if abs(ref - opt) <= 1e-5 * max(1.0, abs(opt)):                     # the reference solved it too
        assert abs(obj - ref) <= 1e-6 * max(1.0, abs(ref))
    else:
        assert name in ("KB2", "SCORPION")


# General-form files that do NOT converge from the reference's start x = s = y = 1 on this path, with the status they end
# in (2 = iteration cap of the driver, 999; 3 = NaN).  Their trajectories are chaotic, so which of them
# converge depends on summation orders: STANDATA converged in 190 iterations until round 2 regrouped the triangular solves
# of small handles.  They stay listed so that the NEXT change of a summation order shows up here as a diff instead of
# being curated out of the parity list above.
GENERAL_EXPECTED_UNCONVERGED = {"STANDATA": 3, "SHELL": 2, "SCAGR25": 3}    # round 3 (profiles/r03_general_form_unconverged_status.txt): NaN at 673, cap 999, NaN at 361


@pytest.mark.parametrize("name", sorted(GENERAL_EXPECTED_UNCONVERGED))
def test_general_form_unconverged_files_keep_their_status(golden_dir, name):
    from interiorpointmethod_amd import general_form as G
    z = np.load(os.path.join(golden_dir, "general", name + ".npz"))

    def mat(prefix):
        if prefix + "_none" in z.files:
            return None
        return sparse.csc_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]),
                                 shape=tuple(int(v) for v in z[prefix + "_shape"]))
    kw = dict(c=z["c"], Aineq=mat("Aineq"), bineq=z["bineq"] if "bineq" in z.files else None, Aeq=mat("Aeq"),
              beq=z["beq"] if "beq" in z.files else None, lb=z["lb"], ub=z["ub"], tol=1e-8, return_info=True)
    obj, info = G.new_interior_sparse(**kw)
    assert info["status"] in (2, 3)
    want = GENERAL_EXPECTED_UNCONVERGED[name]
    assert want is None or info["status"] == want, (name, info["status"], info["iterations"])
    obj2, info2 = G.new_interior_sparse(**kw)                     # chaotic, but deterministic
    assert info2["status"] == info["status"] and info2["iterations"] == info["iterations"]
    _, info_m = G.new_interior_sparse(start="mehrotra", **kw)      # and solvable: from the optional robust start
    opt = float(z["netlib_optimum"])
    assert info_m["status"] == 1 and abs(info_m["objective"] - opt) <= 1e-5 * max(1.0, abs(opt))


def test_two_level_blocking_option(monkeypatch):
    """Grouped Cholesky steps with K = 128*gs trailing updates (default: groups of 2 from 48 blocks on; forced here at 9
    and 16 blocks with groups of 2, 3 and 4, 3 not dividing the block count): same factor as the one-level schedule up
    to rounding, same solve."""
    rng = np.random.default_rng(21)
    for m in (1100, 2048):
        M = rng.standard_normal((m, m + 50))
        B = M @ M.T + 0.5 * np.eye(m)
        rhs = rng.standard_normal(m)
        out = {}
        for gs in ("1", "2", "3", "4"):
            monkeypatch.setenv("IPM_GROUP_STEPS", gs)
            with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
                z, nfix = sv.solve_linear(B, rhs)
                out[gs] = (z.ravel(), sv.get_factor())
            assert nfix == 0 and np.linalg.norm(B @ out[gs][0] - rhs) / np.linalg.norm(rhs) < 1e-10
            assert rel(out[gs][1], out["1"][1]) < 1e-11
        assert rel(out["4"][1], np.linalg.cholesky(B)) < 1e-11
    A, b, c = synthetic_lp(1100, 2300, seed=3)
    res = {}
    for gs in ("1", "2", "4"):
        monkeypatch.setenv("IPM_GROUP_STEPS", gs)
        with ipm.IpmSolver(A, b, c) as sv:
            sv.init_state(0.0)
            res[gs] = sv.solve(tol=1e-8, max_iter=200)
        assert res[gs]["status"] == 1 and res[gs]["iterations"] == res["1"]["iterations"]
        assert abs(res[gs]["objective"] - res["1"]["objective"]) <= 1e-9 * (1 + abs(res["1"]["objective"]))


def test_bulk_update_kernel_bit_identical_to_generic(monkeypatch):
    """chol_update_kernel (adat_syrk stage schedule, buffer loads; csrc/chol_update_f64.h) against the generic
    gemm_nt_f64_kernel<128,128,16,2,2> it replaced for the bulk trailing update (IPM_BULK_VARIANT=7): same tiling and
    summation order, so the factor must be bitwise equal -- one-level (K = 128 lower updates), groups of 3 (rectangular
    K = 128 windows + deferred K = 384 updates), with and without the look-ahead."""
    rng = np.random.default_rng(33)
    m = 1700
    M = rng.standard_normal((m, m + 40))
    B = M @ M.T + 0.5 * np.eye(m)
    for env in ({}, {"IPM_GROUP_STEPS": "3"}, {"IPM_LOOKAHEAD": "0"}):
        L = {}
        for variant in ("0", "7"):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            monkeypatch.setenv("IPM_BULK_VARIANT", variant)
            with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
                _, nfix = sv.solve_linear(B, np.ones(m))
                L[variant] = sv.get_factor().copy()
            assert nfix == 0
        for k in env:
            monkeypatch.delenv(k)
        assert np.array_equal(L["0"], L["7"]), env
        assert rel(L["0"], np.linalg.cholesky(B)) < 1e-11


def test_block_step_and_grouped_substitutions_agree(monkeypatch):
    """The two substitution paths of the dense-tile factor -- one launch per 128-row block step, and explicit inverses of the
    1024-row groups (ragged: leftover blocks step by step) -- solve the same system: block counts that are no multiple of the group
    size (3 ... 13 blocks) and one that is (8); residual 1e-10 each, the two solutions agree to 1e-9."""
    rng = np.random.default_rng(44)
    for m in (300, 850, 1024, 1600):
        M = rng.standard_normal((m, m + 30))
        B = M @ M.T + 0.5 * np.eye(m)
        rhs = rng.standard_normal(m)
        z = {}
        for grouped in ("1", "0"):
            monkeypatch.setenv("IPM_GROUPED_TRSV", grouped)
            with ipm.IpmSolver(np.eye(m, 1), np.zeros(m), np.zeros(1)) as sv:
                z[grouped], nfix = sv.solve_linear(B, rhs)
            assert nfix == 0
            assert np.linalg.norm(B @ z[grouped].ravel() - rhs) / np.linalg.norm(rhs) < 1e-10
        assert rel(z["1"], z["0"]) < 1e-9, m


def test_normal_solve_entry(golden_dir):
    """ipm_normal_solve: (A diag(d) A^T) z = rhs with the handle's own A, dense and sparse, factor reuse."""
    rng = np.random.default_rng(8)
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "SC205.npz"))
    Ad = A.toarray()
    m, n = Ad.shape
    d = 10.0 ** rng.uniform(-2, 2, n)
    r1, r2 = rng.standard_normal(m), rng.standard_normal(m)
    for mat, kw in ((A, {}), (Ad, {}), (A, dict(reorder="rcm"))):
        with ipm.IpmSolver(mat, b, c, **kw) as sv:
            z1 = sv.normal_solve(r1, d)
            z2 = sv.normal_solve(r2, reuse_factor=True)
            z3 = sv.normal_solve(r2)                                  # d = None: A A^T
        B = (Ad * d) @ Ad.T
        assert np.linalg.norm(B @ z1 - r1) / np.linalg.norm(r1) < 1e-9
        assert np.linalg.norm(B @ z2 - r2) / np.linalg.norm(r2) < 1e-9
        assert np.linalg.norm(Ad @ (Ad.T @ z3) - r2) / np.linalg.norm(r2) < 1e-9


def test_qap15_mehrotra_mode(golden_dir):
    """BASELINE config 3 in the optional robust mode: the least-squares start finds 548 of QAP15's 6330 rows dependent
    (guarded pivots of A A^T), switches the 1e-14 Tikhonov shift on for this LP only, and the loop converges to the
    Netlib optimum 1040.994041 in about 25 iterations (default mode: test_qap15_config3_objective / _regularized)."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "QAP15.npz"))
    x, y, s, info = ipm.solve_with_info(A, b, c, tol=1e-8, max_iter=300, start="mehrotra")
    assert info["status"] == 1 and info["iterations"] <= 40
    assert abs(info["objective"] - cTlb - 1040.994041) <= 1e-6 * 1040.994041
    assert info["rp"] <= 1e-8 and info["rd"] <= 1e-8


def test_mehrotra_start_matches_numpy(golden_dir):
    """The start point itself against a dense NumPy evaluation of Mehrotra's formulas."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "SC205.npz"))
    Ad, bb, cc = A.toarray(), b.ravel(), c.ravel()
    G = Ad @ Ad.T
    x = Ad.T @ np.linalg.solve(G, bb)
    y = np.linalg.solve(G, Ad @ cc)
    s = cc - Ad.T @ y
    x = x + max(-1.5 * x.min(), 0.0); s = s + max(-1.5 * s.min(), 0.0)
    xs = 0.5 * (x @ s)
    x = x + xs / s.sum(); s = s + xs / x.sum()
    with ipm.IpmSolver(A, b, c) as sv:
        x0, y0, s0 = sv.mehrotra_start()
    assert rel(x0, x) < 1e-9 and rel(y0, y) < 1e-9 and rel(s0, s) < 1e-9 and x0.min() > 0 and s0.min() > 0


@pytest.mark.parametrize("name", ["AFIRO", "ADLITTLE", "25FV47", "SCAGR25", "SHARE1B", "ISRAEL", "BNL2", "STOCFOR2"])
def test_mehrotra_start_option(golden_dir, name):
    """start="mehrotra" (optional mode; NOT the reference's start): converges to the Netlib optimum
    (the table the reference carries, tests/golden/netlib_optima.json) -- on five of these eight the reference's start
    x = s = 1 runs into the iteration cap -- in fewer iterations than the reference start where both converge."""
    import json
    opt = json.load(open(os.path.join(golden_dir, "netlib_optima.json")))[name]
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    x, y, s, info = ipm.solve_with_info(A, b, c, tol=1e-8, max_iter=300, start="mehrotra")
    assert info["status"] == 1 and abs(info["objective"] - cTlb - opt) <= 1e-6 * max(1.0, abs(opt))
    assert np.all(x > 0) and np.all(s > 0)
    if name in ("AFIRO", "STOCFOR2"):
        _, _, _, ref = ipm.solve_with_info(A, b, c, tol=1e-8, max_iter=300)
        assert ref["status"] == 1 and info["iterations"] < ref["iterations"]


def test_general_form_all_fixtures_with_mehrotra_start(golden_dir):
    """The 40 general-form fixtures with <= 1200 variables (benchmarks_full: inequality and equality rows,
    nonzero lower and finite upper bounds) through the front end with the optional Mehrotra start: every one converges
    to the Netlib optimum the reference lists (gap tolerance of this driver is 1e-6, so 1e-5 relative here).  The
    reference's own driver reaches the optimum on 13 of them."""
    import glob
    from interiorpointmethod_amd import general_form as G
    files = sorted(glob.glob(os.path.join(golden_dir, "general", "*.npz")))
    done = 0
    for f in files:
        z = np.load(f)
        if z["c"].shape[0] > 1200:          # the larger files: tools/general_report.py / bench.py --netlib-set general
            continue
        done += 1

        def mat(prefix):
            if prefix + "_none" in z.files:
                return None
            return sparse.csc_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]),
                                     shape=tuple(int(v) for v in z[prefix + "_shape"]))
        obj, info = G.new_interior_sparse(c=z["c"], Aineq=mat("Aineq"), bineq=z["bineq"] if "bineq" in z.files else None,
                                          Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, lb=z["lb"], ub=z["ub"],
                                          tol=1e-8, return_info=True, start="mehrotra")
        opt = float(z["netlib_optimum"])
        assert info["status"] == 1, (os.path.basename(f), info["status_name"])
        assert abs(obj - opt) <= 1e-5 * max(1.0, abs(opt)), (os.path.basename(f), obj, opt)
    assert done >= 40


SMALL_LPS = ["AFIRO", "ADLITTLE", "KB2", "SC105", "SC50A", "SC50B", "SCSD1", "SHARE1B", "SHARE2B", "STOCFOR1"]


@pytest.mark.parametrize("name", SMALL_LPS)
def test_fused_small_lp_path(golden_dir, monkeypatch, name):
    """The 10 Netlib files with m <= 128 run their whole loop in ONE launch of one workgroup (small_lp.h).  Against
    the multi-kernel path (IPM_FUSED_SMALL=0) on the same LP: same status; where both converge the same objective
    to 1e-8 and iteration counts within 2 (summation orders differ, trajectories are chaotic: SURVEY H1); bitwise
    repeatable; history, iterate() and the stop test on the host behave as on the other path.  The reference
    comparison itself is test_netlib_parity (8 of these 10 are in the parity set and now take the fused path)."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", name + ".npz"))
    Af, bf, cf = O.as_float64_problem(A, b, c)
    with ipm.IpmSolver(A, b, c) as sv:
        assert sv.schedule()["fused_small"] == 1
        sv.init_state(1.0)
        st = sv.solve(tol=1e-8, max_iter=300)
        x, y, s = sv.get_state()
        hist = sv.history()
        sv.init_state(1.0)
        st_b = sv.solve(tol=1e-8, max_iter=300)
        assert st_b["iterations"] == st["iterations"] and np.array_equal(sv.get_state()[0], x, equal_nan=True)   # reproducible (SHARE1B ends in NaN, like the reference's loop on it)
        sv.init_state(1.0)
        it2 = sv.iterate(2)
        x2, y2, s2 = sv.get_state()
        assert it2["iterations"] == 2 and np.isclose(it2["gap"], float((x2.T @ s2).item()), rtol=1e-12)
        assert np.isclose(it2["rp_norm"], np.linalg.norm(Af @ x2 - bf), rtol=1e-9, atol=1e-12)
    monkeypatch.setenv("IPM_FUSED_SMALL", "0")
    with ipm.IpmSolver(A, b, c) as mk:
        assert mk.schedule()["fused_small"] == 0
        mk.init_state(1.0)
        ref = mk.solve(tol=1e-8, max_iter=300)
        mk.init_state(1.0)
        mk.iterate(2)
        xm, ym, sm = mk.get_state()
    assert rel(x2, xm) < 1e-9 and rel(y2, ym) < 1e-9 and rel(s2, sm) < 1e-9            # two iterations: rounding only
    assert st["status"] == ref["status"], (st["status"], ref["status"])
    assert len(hist) == min(st["iterations"], 1024) and all(r["k"] == i for i, r in enumerate(hist))
    if st["status"] == 1:
        assert abs(st["iterations"] - ref["iterations"]) <= 2
        assert abs(st["objective"] - ref["objective"]) <= 1e-8 * max(1.0, abs(ref["objective"]))
        assert not O.check_optimality(Af, bf, cf, x, y, s, 1e-8, 1e-8, 1e-8)
    if name == "AFIRO":
        assert st["solve_ms"] < 4.0, st["solve_ms"]         # 93 iterations; the multi-kernel path needs ~10 ms
        print("AFIRO fused %.3f ms, multi-kernel %.3f ms" % (st["solve_ms"], ref["solve_ms"]))


def test_history_and_iterate_statistics(golden_dir):
    """ipm_get_history: one record per iteration (the line the reference prints, main.py:808-809/:1186), consistent
    with the final statistics; ipm_iterate's statistics describe the state ipm_get_state returns."""
    A, b, c, cTlb, valid = load_npz_problem(os.path.join(golden_dir, "netlib", "SC50A.npz"))
    Af, bf, cf = O.as_float64_problem(A, b, c)
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(1.0)
        st = sv.solve(tol=1e-8, max_iter=500)
        h = sv.history()
        assert st["status"] == 1 and len(h) == st["iterations"] and [r["k"] for r in h] == list(range(len(h)))
        assert np.isclose(h[0]["objective"], float(np.sum(cf)), rtol=1e-14) and h[0]["mu"] == 1.0   # x = s = 1 at the start
        assert all(0.0 < r["alpha_p"] <= 0.91 and 0.0 < r["alpha_d"] <= 0.91 for r in h)   # eta = 0.91, main.py:607
        assert h[-1]["gap"] > st["gap"] and st["objective_last_finite"] == st["objective"]
        # ipm_iterate: statistics of the state reached, not of the one before the last step
        sv.init_state(1.0)
        st3 = sv.iterate(3)                     # the count restarts with the newly set iterate
        x, y, s = sv.get_state()
        assert st3["iterations"] == 3
        assert np.isclose(st3["objective"], float((cf.T @ x).item()), rtol=1e-13)
        assert np.isclose(st3["gap"], float((x.T @ s).item()), rtol=1e-12)
        assert np.isclose(st3["rp_norm"], np.linalg.norm(Af @ x - bf), rtol=1e-9, atol=1e-13)
        assert np.isclose(st3["rd_norm"], np.linalg.norm(Af.T @ y + s - cf), rtol=1e-9, atol=1e-13)
        h3 = sv.history()
        assert len(h3) == 3 and h3[0]["objective"] == h[0]["objective"] and h3[2]["alpha_p"] == h[2]["alpha_p"]
        assert sv.iterate(2)["iterations"] == 5 and len(sv.history()) == 5      # ... and continues over further calls


def test_nan_solve_returns_last_finite_objective():
    """new_interior_sparse returns the last finite objective when the iterate goes NaN (main.py:1227-1233).  An
    infeasible LP (x1 + x2 = -1, x >= 0) drives the loop there."""
    from interiorpointmethod_amd import general_form as G
    Aeq = sparse.csc_matrix(np.array([[1.0, 1.0]]))
    obj, info = G.new_interior_sparse(c=np.array([1.0, 2.0]), Aeq=Aeq, beq=np.array([-1.0]), lb=np.zeros(2),
                                      ub=np.full(2, np.inf), tol=1e-8, return_info=True)
    if info["status"] == 3:
        assert np.isfinite(obj) and obj == info["objective_last_finite"] and not np.isfinite(info["objective"])
    else:
        assert info["status"] == 2 and np.isfinite(info["objective_last_finite"])


def test_two_default_handles_from_two_threads():
    """Two DEFAULT handles (no IPM_FLAG_NO_DEVICE_POLLING) driven from two host threads on one GPU.  The
    library counts live handles per device and uses stream events while more than one exists; a poll that times out
    anyway is rolled back and repeated with events (ipm_get_schedule: timeouts_recovered) -- never an error, and the
    results equal the single-handle run bit for bit (the synchronisation mechanism does not change arithmetic)."""
    import threading
    A, b, c = synthetic_lp(1536, 3072, seed=5)               # 12 blocks: look-ahead with hand-offs at every step
    with ipm.IpmSolver(A, b, c) as one:
        assert one.schedule()["live_handles"] == 1 and one.schedule()["device_polling"] == 1
        one.init_state(0.0)
        ref = one.solve(tol=1e-8, max_iter=200)
        xref = one.get_state()[0]
        assert one.schedule()["counter_steps"] > 0
    out, errs = {}, []

    def run(tag):
        try:
            import torch
            with torch.cuda.stream(torch.cuda.Stream()):
                with ipm.IpmSolver(A, b, c) as sv:
                    barrier.wait()
                    sv.init_state(0.0)
                    st = sv.solve(tol=1e-8, max_iter=200)
                    out[tag] = (st, sv.get_state()[0], sv.schedule())
                    barrier.wait()
        except Exception as e:                                 # noqa: BLE001
            errs.append(e)
            barrier.abort()

    barrier = threading.Barrier(2)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not errs, errs
    for tag in (0, 1):
        st, x, sched = out[tag]
        assert sched["live_handles"] == 2 and sched["device_polling"] == 0
        assert st["status"] == 1 and st["iterations"] == ref["iterations"] and st["objective"] == ref["objective"]
        assert np.array_equal(x, xref)


def _solve_checked(A, b, c, y0=0.0):
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(y0)
        st = sv.solve(tol=1e-8, max_iter=200)
        x, y, s = sv.get_state()
        sched = sv.schedule()
    return st, x, y, s, sched


def _check_lp_properties(A, b, c, st, x, y, s):
    """Size-independent properties of a converged primal-dual pair (used where the reference cannot run)."""
    assert st["status"] == 1
    assert np.linalg.norm(A @ x - b) / (1 + np.linalg.norm(b)) < 1e-8
    assert np.linalg.norm(A.T @ y + s - c) / (1 + np.linalg.norm(c)) < 1e-8
    assert np.all(x > 0) and np.all(s > 0) and (x.T @ s).item() <= 1e-8
    pobj, dobj = (c.T @ x).item(), (b.T @ y).item()
    assert abs(pobj - dobj) <= 1e-6 * max(1.0, abs(pobj))


def test_dense_6200x9000_default_two_level(monkeypatch):
    """49 blocks: the size from which the two-level Cholesky (groups of 3) is the schedule of the SERIAL path (formation, then
    factorization; since round 4 the default at this size is the fused launch, which this test also runs and compares).  Same
    iteration count and objective as the one-level factor (IPM_TWO_LEVEL=0) and the LP-level properties.  49 is no multiple
    of the 8-block groups of the triangular solves: six full groups get their explicit inverses, the last block is solved as
    a block step (ragged groups, round 3) -- same answer as the block-step substitutions alone (IPM_RAGGED_GROUPS=0)."""
    A, b, c = synthetic_lp(6200, 9000, seed=2)
    stf, xf, yf, sf, schedf = _solve_checked(A, b, c)
    assert schedf["blocks"] == 49 and schedf["fused_factor"] == 1 and schedf["timeouts_recovered"] == 0
    _check_lp_properties(A, b, c, stf, xf, yf, sf)
    monkeypatch.setenv("IPM_FUSED_FACTOR", "0")
    st, x, y, s, sched = _solve_checked(A, b, c)
    assert sched["blocks"] == 49 and sched["group_steps"] == 3 and sched["grouped_trsv"] == 1 and sched["fused_factor"] == 0
    _check_lp_properties(A, b, c, st, x, y, s)
    assert stf["iterations"] == st["iterations"] and abs(stf["objective"] - st["objective"]) <= 1e-9 * max(1.0, abs(st["objective"]))
    assert rel(xf, x) < 1e-6
    monkeypatch.setenv("IPM_TWO_LEVEL", "0")
    st1, x1, _, _, sched1 = _solve_checked(A, b, c)
    assert sched1["group_steps"] == 1 and st1["iterations"] == st["iterations"]
    assert abs(st1["objective"] - st["objective"]) <= 1e-9 * max(1.0, abs(st["objective"]))
    assert rel(x, x1) < 1e-6
    monkeypatch.delenv("IPM_TWO_LEVEL")
    monkeypatch.setenv("IPM_RAGGED_GROUPS", "0")
    st2, x2, _, _, sched2 = _solve_checked(A, b, c)
    assert sched2["grouped_trsv"] == 0 and st2["iterations"] == st["iterations"]
    assert abs(st2["objective"] - st["objective"]) <= 1e-9 * max(1.0, abs(st["objective"])) and rel(x, x2) < 1e-6


def test_dense_16384x32768_config5(monkeypatch):
    """BASELINE.json configs[4]: dense synthetic LP m=16384 n=32768 (A 4.3 GB, B 2.1 GB).  The reference cannot run
    this size (its (m+2n)^2 KKT matrix is 53.7 GB), so the pins are the LP-level properties -- primal and
    dual feasibility, complementarity, zero duality gap -- bitwise repeatability, and agreement with the same solve
    under the one-level factorization.  Asserts that the default schedule really is the one this size is meant to
    exercise: 128 blocks, groups of 4, grouped triangular solves, and BOTH hand-off kinds (stream events for the
    > 1024-tile trailing updates of the early steps, device counters for the late ones)."""
    A, b, c = synthetic_lp(16384, 32768, seed=0)
    st, x, y, s, sched = _solve_checked(A, b, c)
    assert sched["blocks"] == 128 and sched["group_steps"] == 4 and sched["grouped_trsv"] == 1
    assert sched["device_polling"] == 1 and sched["event_steps"] > 0 and sched["counter_steps"] > 0
    assert sched["timeouts_recovered"] == 0
    _check_lp_properties(A, b, c, st, x, y, s)
    assert 15 <= st["iterations"] <= 40
    st2, x2, _, _, _ = _solve_checked(A, b, c)
    assert st2["iterations"] == st["iterations"] and np.array_equal(x, x2)          # bitwise reproducible
    monkeypatch.setenv("IPM_TWO_LEVEL", "0")
    st1, x1, _, _, sched1 = _solve_checked(A, b, c)
    assert sched1["group_steps"] == 1 and st1["iterations"] == st["iterations"]
    assert abs(st1["objective"] - st["objective"]) <= 1e-9 * max(1.0, abs(st["objective"]))
    assert rel(x, x1) < 1e-6


def test_netlib_suite_batched_config4(golden_dir):
    """BASELINE.json configs[3]: ALL 73 valid benchmarks/ LPs through batch.run_batch with EIGHT LPs in flight -- what
    bench.py runs -- (the driver loop of script.py:147-173, tol=1e-8, cap 300).  Every record is a solver status
    (converged / cap / NaN: the reference itself converges on 26 only) -- no library error -- the 26
    parity LPs reproduce the reference's objectives (e2e_*.npz) to 1e-6 relative, the table equals the one-at-a-time
    run, and the library's hidden recoveries stayed hidden because there were none: no hand-off poll timed out and was
    rolled back (timeouts_recovered), no sparse-factor sweep ran as one workgroup (serial_launches), in either run."""
    import glob
    from interiorpointmethod_amd import batch
    names, probs = [], []
    for f in sorted(glob.glob(os.path.join(golden_dir, "netlib", "*.npz"))):
        A, b, c, cTlb, valid = load_npz_problem(f)
        if valid:
            names.append(os.path.basename(f)[:-4]); probs.append((A, b, c))
    assert len(names) == 73
    par, _ = batch.run_batch(probs, tol=1e-8, max_iter=300, workers=8)
    assert np.array_equal(par[:, 0], np.arange(73))
    assert set(par[:, 1].tolist()) <= {1.0, 2.0, 3.0}, [(names[int(r[0])], r[1]) for r in par if r[1] not in (1, 2, 3)]
    F = batch.RECORD_FIELDS
    assert not par[:, F.index("timeouts_recovered")].any(), [names[int(r[0])] for r in par if r[F.index("timeouts_recovered")]]
    assert not par[:, F.index("serial_launches")].any(), [names[int(r[0])] for r in par if r[F.index("serial_launches")]]
    assert np.all(par[:, F.index("solve_seconds")] > 0) and np.all(par[:, F.index("setup_seconds")] > 0)
    conv = {names[int(r[0])] for r in par if r[1] == 1.0}
    assert set(PARITY_FAST) <= conv and {"QAP8", "QAP12", "QAP15"} <= conv
    for r in par:
        nm = names[int(r[0])]
        if nm in PARITY_FAST:
            ref = float(np.load(os.path.join(golden_dir, "e2e_%s.npz" % nm))["objective"])
            assert abs(r[3] - ref) <= 1e-6 * max(1.0, abs(ref)), (nm, r[3], ref)
    seq, _ = batch.run_batch(probs, tol=1e-8, max_iter=300, workers=1)
    assert not seq[:, F.index("timeouts_recovered")].any() and not seq[:, F.index("serial_launches")].any()
    same = (seq[:, 3] == par[:, 3]) | (np.isnan(seq[:, 3]) & np.isnan(par[:, 3]))
    assert np.array_equal(seq[:, 1:3], par[:, 1:3]) and np.all(same)
    assert batch.summarize(par)["total_iterations"] == batch.summarize(seq)["total_iterations"]
    # what bench.py runs by default (lockstep="auto": with 61 LPs of more than 128 rows on one GPU the LOCKSTEP batches):
    # the same LPs converge to the same objectives in the same number of iterations.  (Inside a batch an LP of up to 3500 rows takes
    # the dense-tile factor even where a lone solve takes the sparse one, so the LPs that end at the cap or in NaN may do so after a
    # different number of iterations; the bit-for-bit comparison of the same handle alone / in a batch is tests/test_gpu_lockstep.py.)
    assert batch.lockstep_wanted(probs, world=1, workers=8, mode="auto")
    lock, _ = batch.run_batch(probs, tol=1e-8, max_iter=300, workers=8, lockstep="auto")
    assert np.array_equal(lock[:, 0], np.arange(73)) and set(lock[:, 1].tolist()) <= {1.0, 2.0, 3.0}
    assert not lock[:, F.index("timeouts_recovered")].any() and not lock[:, F.index("serial_launches")].any()
    assert {names[int(r[0])] for r in lock if r[1] == 1.0} == conv
    for r, q in zip(lock, par):
        if q[1] == 1.0:
            assert abs(r[3] - q[3]) <= 1e-8 * max(1.0, abs(q[3])) and abs(r[2] - q[2]) <= 2, (names[int(r[0])], r[2:4], q[2:4])


def test_results_table_against_reference_log(tmp_path):
    """tools/netlib_report.py (the table of script.py:139-198) over general-form inputs the reference's own log
    covers: the "Interi" column must print what conclusion1.txt:3,6 printed for AFIRO and BANDM (2 decimals), and
    the Netlib and SciPy columns agree with them."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("netlib_report", os.path.join(root, "tools", "netlib_report.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    from interiorpointmethod_amd import general_form as GF
    solve = lambda c, Aineq, bineq, Aeq, beq, lb, ub: GF.new_interior_sparse(                   # noqa: E731
        c=c, Aineq=Aineq, bineq=bineq, Aeq=Aeq, beq=beq, lb=lb, ub=ub, tol=1e-6)
    rows = R.run_general(["AFIRO", "BANDM"], solve)
    out = os.path.join(tmp_path, "conclusion_gpu.txt")
    R.write_table(rows, out)
    lines = open(out, newline="").read().split("\r\n")
    got = {ln.split()[0]: ln.split()[3:] for ln in lines[1:] if ln}
    assert got["AFIRO"] == ["-464.75", "-464.75", "-464.75"]          # conclusion1.txt:3
    assert got["BANDM"] == ["-158.63", "-158.63", "-158.63"]          # conclusion1.txt:6


def test_batch_two_at_a_time_same_records(golden_dir):
    """Batched mode with two LPs in flight per GPU (host threads, own streams, IPM_FLAG_NO_DEVICE_POLLING): the
    records equal the one-at-a-time run bit for bit -- only the synchronisation mechanism differs."""
    from interiorpointmethod_amd import batch
    names = ["AFIRO", "SC50A", "BANDM", "SCSD6", "SHARE2B", "STOCFOR1", "SC205", "E226"]
    probs = [load_npz_problem(os.path.join(golden_dir, "netlib", nm + ".npz"))[:3] for nm in names]
    seq, _ = batch.run_batch(probs, tol=1e-8, max_iter=300, workers=1)
    par, _ = batch.run_batch(probs, tol=1e-8, max_iter=300, workers=2)
    assert np.array_equal(seq[:, 0], np.arange(len(names))) and np.array_equal(par[:, 0], seq[:, 0])
    assert np.all(seq[:, 1] == 1.0)
    assert np.array_equal(par[:, 1:4], seq[:, 1:4])            # status, iterations, objective


def test_rccl_branch_with_one_rank(golden_dir, tmp_path):
    """The RCCL code path on the one GPU a test box has: a process group of ONE rank over backend "nccl" (= RCCL on ROCm),
    (i) batch.gather_records / batch._gather_sparse pushed through dist.all_gather with DEVICE tensors of the record
    shape (float64 (cap, NF)), (ii) a batched solve with the self-scheduling counter on a TCPStore and the records
    gathered on the device, (iii) bench.py --workload netlib under torch.distributed.run --nproc-per-node 1 with
    IPM_BENCH_FORCE_DIST=1.  Proves the library loads, the gathers work and the store path is sound before a driver
    hands the job eight GPUs; own processes, so the test session's torch state is untouched."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=root)
    code = r'''
import os, numpy as np, torch, torch.distributed as dist
from interiorpointmethod_amd import batch
from interiorpointmethod_amd.matio import load_npz_problem
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
local = np.column_stack([np.arange(5.0)[::-1], rng.standard_normal((5, batch.NF - 1))])
out = batch.gather_records(local, [5], dist=dist, device=dev)              # padded (cap, NF) float64 through all_gather
assert np.array_equal(out, local[::-1])
tab = np.full((7, batch.NF), -1.0); tab[[1, 4]] = rng.standard_normal((2, batch.NF)); tab[[1, 4], 0] = [1, 4]
got = batch._gather_sparse(tab, dist, device=dev)
assert np.array_equal(got, tab)
store = batch.make_store(0, 1, host="127.0.0.1", port=int(os.environ["MASTER_PORT"]) + 1)
names = ["AFIRO", "SC50A", "BANDM", "SCSD6", "STOCFOR2"]
probs = [load_npz_problem(os.path.join(os.environ["GOLDEN"], "netlib", nm + ".npz"))[:3] for nm in names]
for sched in ("dynamic", "static"):
    rec, _ = batch.run_batch(probs, device=0, dist=dist, store=store, schedule=sched, workers=2, gather_device=dev,
                             collective_at_world_one=True, tol=1e-8, max_iter=300)
    assert np.array_equal(rec[:, 0], np.arange(5)) and np.all(rec[:, 1] == 1.0), rec[:, :3]
ref, _ = batch.run_batch(probs, device=0, tol=1e-8, max_iter=300)
assert np.array_equal(ref[:, 1:4], rec[:, 1:4])
dist.barrier()
dist.destroy_process_group()
print("RCCL_ONE_RANK_OK")
'''
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(env, GOLDEN=golden_dir))
    assert out.returncode == 0 and "RCCL_ONE_RANK_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port2 = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port2), os.path.join(root, "bench.py"), "--workload", "netlib", "--netlib-set", "parity",
           "--max-m", "1500", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, IPM_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert "backend nccl" in line["config"]["workload"] and "TCPStore" in line["config"]["workload"]
    assert line["summary"]["converged"] == line["summary"]["n"] >= 20 and line["summary"]["errors"] == 0
    assert line["summary"]["timeouts_recovered"] == 0 and line["summary"]["serial_launches"] == 0


def test_bench_plain_and_full_lines(tmp_path):
    """bench.py, dense workload, in its own processes: a plain run prints the contract keys and the roofline of its timed
    steps and dumps the iterate, but runs none of the extras; --full adds the untimed phase pass and the objective check
    (here against a second handle: no reference trajectory is committed for this size)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--m", "1024", "--n", "2048", "--steps", "3",
            "--warmup", "1"]

    def run(extra):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        lines = out.stdout.strip().splitlines()
        detail = [ln for ln in lines if ln.startswith("BENCH_DETAIL ")]
        assert len(detail) == 1
        return json.loads(lines[-1]), json.loads(detail[0][len("BENCH_DETAIL "):])

    plain, plain_detail = run(["--dump-outputs", str(tmp_path / "dump")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    for k in ("objective_check", "cpu_baseline", "cpu_baseline_reference_algorithm", "netlib_all", "netlib"):
        assert k not in plain, k
    for nm, size in (("x", 2048), ("y", 1024), ("s", 2048)):
        v = np.load(tmp_path / "dump" / (nm + ".npy"))
        assert v.size == size and np.all(np.isfinite(v))
    assert not set(("factor", "trisolve", "other")) & set(plain_detail["phases_ms_per_step"])
    full, full_detail = run(["--full", "--no-netlib", "--no-cpu-baseline"])
    assert full["objective_check"] == "ok" and "cpu_baseline" not in full and "netlib_all" not in full
    assert set(("factor", "trisolve", "other")) <= set(full_detail["phases_ms_per_step"])


def test_plain_c_driver():
    """examples/c_driver.c: the C ABI from plain C in its own process (no Python, no torch; the library allocates its
    workspace and stream): the reference's ex1 optimum -775 (main.py:1253) and a random 300 x 700 LP."""
    import subprocess
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "c_driver")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("libipm_hip ABI 4")
    ex1 = dict(zip(lines[1].split()[1::2], lines[1].split()[2::2]))
    assert ex1["status"] == "1" and abs(float(ex1["objective"]) + 775.0) < 1e-6 and int(ex1["iterations"]) == 17
    assert "random 300x700: status 1" in lines[2]


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


@pytest.mark.parametrize("fused", ["0", "force"])
def test_padding_rows_of_the_block_inverses_are_the_identity(monkeypatch, fused):
    """potrf_diag factors only the 16-wide panels of a partial last block that hold rows of the LP and FILLS the
    inverse of the padding rows with the identity; the fill raced with the block load in LDS (fixed with a barrier in round 4).
    m = 1100 = 8 x 128 + 76: the last block has 5 factored panels (80 rows), rows 80 .. 127 of inv(L_88) must be EXACTLY e_i, rows
    76 .. 79 (padding inside the last factored panel: unit diagonal of B) as well, on the serial chain and on the fused launch; and
    the inverse of the real part inverts L (1e-12)."""
    import ctypes as C
    from interiorpointmethod_amd import _lib
    m, n = 1100, 2300
    A, b, c = synthetic_lp(m, n, seed=7)
    monkeypatch.setenv("IPM_FUSED_FACTOR", fused)
    with ipm.IpmSolver(A, b, c) as sv:
        sv.init_state(0.0)
        sv.iterate(2)
        assert sv.schedule()["fused_factor"] == (1 if fused == "force" else 0)
        L = sv.get_factor()
        inv = np.zeros((128, 128))
        sv._check(_lib.load().ipm_debug_get_block_inverse(sv._h, 8, inv.ctypes.data_as(C.POINTER(C.c_double))))
    real = m - 8 * 128
    assert np.array_equal(inv[real:, :], np.eye(128)[real:, :])                       # exact unit rows on the padding
    assert np.array_equal(inv[:, real:], np.eye(128)[:, real:])
    L88 = L[8 * 128:, 8 * 128:]
    assert np.max(np.abs(inv[:real, :real] @ L88 - np.eye(real))) < 1e-12
    assert np.all(np.triu(inv, 1) == 0.0)
