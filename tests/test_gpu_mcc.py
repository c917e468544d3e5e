"""GPU tests (-m gpu) of Gondzio's centrality correctors (csrc/iteration_rules.h mcc_*, vector_ops.h mcc_*_kernel, host_iteration.h
enqueue_corrector_rounds).

One iteration against the oracle.  tests/mcc_oracle.py restates one iteration with K rounds in longdouble; a cell sets the case's
state, runs iterate(1) with K = 1, 2, 3 and compares, element by element, the next (x, y, s, w, z), A^T y, alpha_p, alpha_d and the
direction the device stepped along, recovered as (next - state) / alpha as test_gpu_iteration_edges.check_iteration does for dw,
and the info record (rounds that did work, rounds accepted) against the oracle's decisions.  Shapes: one block with padding
(5 x 65 bounded), one column in the last block (130 x 257 bounded), the unbounded instantiation over three blocks (300 x 513), the
first grid-stride trip with and without bounds (129 x 16385), each as dense ingest and as sparse ingest on the envelope factor
(IPM_FUSED_SMALL=0 where m <= 128), 130 x 257 also on the sparse factor, and the full-step case.  dense/129x16385 rejects its first
round, so K = 2, 3 run dead rounds there; sparse/129x16385 rejects its third.  tests/test_mcc_oracle_host.py asserts the cells'
preconditions (accept margins >= 1e-6 and so on).

Tolerances: the suite's bounds for this seam, test_gpu_iteration_edges._bound: 100 x the maximum that file's first run observed for
the quantity, never below 1e-12.  A round adds one more solve with the same factor to what those bounds were measured on.

Observed maxima on MI355X (first run of this file), per quantity over all cells:
    dx 1.8e-14, x 7.4e-15, s 1.0e-14, y, A^T y 4.5e-15, alpha_p 1.0e-14, alpha_d 8.1e-15                    300 x 513
    ds 2.3e-14, dy, A^T dy 5.8e-15                                                                             full step, 129 x 16385
    w 2.7e-15, z 4.6e-15, dw 8.4e-15, dz 8.6e-15                                                               130 x 257 bounded
  all below the maxima those bounds were derived from (test_gpu_iteration_edges.OBSERVED): a round costs no accuracy.

K = 0 is the old code: a handle on which set_correctors(0) was called and an untouched one are bit-identical after iterate(5).
Repeatability and the overlapped path: dense 2048 x 2304 (16 blocks: residual stream, streamed A^T dy for Mehrotra's two solves) with
K = 3 -- iterate(4) twice from the same state, and once more under IPM_STREAM_AT=0, all bit-identical.
Residue: fresh handles on memory filled with 0x00, 0xFF and left alone give the same bytes with K = 3.
Refusals: a small-path handle and a lockstep handle raise from set_correctors(1), accept set_correctors(0) and stay usable; the
batch front ends raise ValueError; a handle moved to the small path after K > 0 is refused by iterate / solve until K = 0.

End to end (K = 2 at eta = 0.91 and 0.995, tests/golden/dense_syn_256x512.npz and GROW22 with native bounds from Mehrotra's start):
status converged, the returned iterate passes the stop test recomputed in longdouble at the solve's tolerances, and the objective
agrees with the K = 0 solve's within a bound derived from that stop test.  Derivation (stop_test_kernel_body: both iterates have
rp_i = ||(A x_i - b, x_i + w_i - u on U)|| <= e1 (1 + ||(b, u_U)||), rd_i = ||A^T y_i + s_i - z_i - c|| <= e2 (1 + ||c||),
gap_i = x_i.s_i + w_i.z_i <= e3, and x, s, w, z > 0).  With d_i = b.y_i - u.z_i and c = A^T y_k + s_k - z_k - rc_k, A x_i = b + rb_i,
x_i = u - w_i + ru_i on U:
    c.x_i - d_k = y_k.rb_i - z_k.ru_i - rc_k.x_i + (s_k.x_i + z_k.w_i)
For k = i the last term is gap_i; for k != i it is >= 0.  So c.x_1 - d_2 >= -E(2,1), c.x_2 - d_2 <= gap_2 + E(2,2), with
E(k,i) = ||(y_k, z_k)|| rp_i + rd_k ||x_i||, hence c.x_1 - c.x_2 >= -(gap_2 + E(2,1) + E(2,2)), and the same with 1 and 2 exchanged:
    |c.x_1 - c.x_2| <= e3 + 2 e1 (1 + ||(b, u_U)||) max_k ||(y_k, z_k)|| + 2 e2 (1 + ||c||) max_i ||x_i||
Iteration counts are printed (ITERS lines), not asserted.
"""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib
from interiorpointmethod_amd import general_form as G
from interiorpointmethod_amd.workloads import synthetic_lp

import iteration_oracle as IO
import mcc_oracle as M
from test_gpu_iteration_edges import OBSERVED, _bound      # noqa: F401  (the seam's bounds)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _solver(case, as_sparse=False, **opts):
    A = sparse.csc_matrix(case.A) if as_sparse else case.A
    return ipm.IpmSolver(A, case.b, case.c, ub=case.ub(), **opts)


def _srel(got, want):
    want = IO.LD(want)
    return float(abs(IO.LD(got) - want) / abs(want))


def _bits(sv):
    out = [v.tobytes() for v in sv.get_state()]
    if sv.bounded:
        out += [v.tobytes() for v in sv.get_bound_state()]
    return out


def check_round_cell(cell, sv, case, name, K):
    """iterate(1) with K rounds from the case's state against the oracle's K-round run."""
    o = M.oracle(name, K)
    AT = case.A.T
    sv.set_correctors(K)
    sv.set_state(*case.state())
    st = sv.iterate(1)
    info = sv.corrector_info()
    x, y, s = (v.ravel() for v in sv.get_state())
    ap, ad = st["alpha_p"], st["alpha_d"]
    e, bound = {}, {}

    def vec(k, got, want):
        e[k], bound[k] = IO.rel(got, want), _bound(k)

    vec("x", x, o["xn"]); vec("s", s, o["sn"]); vec("y", y, o["yn"]); vec("ATy", AT @ y, o["atyn"])
    e["alpha_p"], bound["alpha_p"] = _srel(ap, o["alpha_p"]), _bound("alpha_p")
    e["alpha_d"], bound["alpha_d"] = _srel(ad, o["alpha_d"]), _bound("alpha_d")
    vec("dx", (x - case.x) / ap, o["dx"]); vec("ds", (s - case.s) / ad, o["ds"]); vec("dy", (y - case.y) / ad, o["dy"])
    vec("ATdy", AT @ ((y - case.y) / ad), o["atdy"])
    if case.bounded:
        w, z = (v.ravel() for v in sv.get_bound_state())
        U = case.U
        vec("w", w, o["wn"]); vec("z", z, o["zn"])
        assert np.all(w[~U] == 0) and np.all(z[~U] == 0)
        vec("dw", (w - case.w) / ap, o["dw"]); vec("dz", (z - case.z) / ad, o["dz"])
    for k in sorted(e):
        print("OBS %s/K=%d %s %.3e" % (cell, K, k, e[k]))
    want = dict(k=K, rounds=o["rounds_run"], accepted=o["rounds_accepted"], iterations=1 if o["rounds_accepted"] else 0)
    print("INFO %s/K=%d %s oracle %s" % (cell, K, info, [r["accepted"] for r in o["rounds"]]))
    assert info == want, (cell, K, info, want)
    bad = {k: v for k, v in e.items() if not v <= bound[k]}
    assert not bad, (cell, K, bad)
    hist = sv.history()
    assert len(hist) == 1 and hist[0]["alpha_p"] == ap and hist[0]["alpha_d"] == ad and st["iterations"] == 1


DENSE_CELLS = [M.cell_name(*sh) for sh in M.SHAPES] + ["full"]
SPARSE_CELLS = [(M.cell_name(*sh, sparse=True), "dense") for sh in M.SHAPES] + [("sparse/130x257b", "sparse")]


@pytest.mark.parametrize("name", DENSE_CELLS)
def test_rounds_dense_ingest(name):
    case = M.get(name)
    with _solver(case) as sv:
        sch = sv.schedule()
        assert not sv.sparse and sch["fused_small"] == 0 and sv.bounded == int(case.U.sum())
        for K in (1, 2, 3):
            check_round_cell(name, sv, case, name, K)


@pytest.mark.parametrize("name,factor", SPARSE_CELLS, ids=["%s-%s" % c for c in SPARSE_CELLS])
def test_rounds_sparse_ingest(name, factor, monkeypatch):
    case = M.get(name)
    if case.m <= 128:
        monkeypatch.setenv("IPM_FUSED_SMALL", "0")
    with _solver(case, as_sparse=True, factor=factor) as sv:
        sch = sv.schedule()
        assert sv.sparse and sv.factor == factor and sch["fused_small"] == 0 and sv.bounded == int(case.U.sum())
        if factor == "sparse":
            assert sv.factor_info()["panels"] >= 1
        for K in (1, 2, 3):
            check_round_cell("%s/factor=%s" % (name, factor), sv, case, name, K)


# ---- K = 0 is the old code -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,as_sparse", [("dense/130x257b", False), ("sparse/300x513", True)])
def test_k0_is_bit_identical_to_an_untouched_handle(name, as_sparse):
    case = M.get(name)
    out = []
    for touch in (False, True):
        with _solver(case, as_sparse=as_sparse) as sv:
            if touch:
                sv.set_correctors(2)
                sv.set_correctors(0)
            sv.set_state(*case.state())
            st = sv.iterate(5)
            assert st["iterations"] == 5
            out.append((_bits(sv), sv.history(), sv.corrector_info()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2] == out[1][2] == dict(k=0, rounds=0, accepted=0, iterations=0)


def test_a_handle_set_back_to_k0_is_the_untouched_handle_again():
    """K = 2 for two iterations, then K = 0 from a newly set state: the iterate and the history are those of a handle that never ran a
    round, and the info record restarts with the iteration count."""
    case = M.get("dense/130x257b")
    with _solver(case) as sv:
        sv.set_state(*case.state())
        sv.iterate(3)
        want = (_bits(sv), sv.history())
    with _solver(case, correctors=2) as sv:
        sv.set_state(*case.state())
        sv.iterate(2)
        assert sv.corrector_info()["rounds"] >= 2
        sv.set_correctors(0)
        sv.set_state(*case.state())
        sv.iterate(3)
        assert (_bits(sv), sv.history()) == want
        assert sv.corrector_info() == dict(k=0, rounds=0, accepted=0, iterations=0)


# ---- repeatability, and the overlapped path --------------------------------------------------------------------------------
def test_rounds_repeat_bitwise_on_the_overlapped_path(monkeypatch):
    A, b, c = synthetic_lp(2048, 2304, seed=7)

    def run(sv):
        sv.init_state(0.0)
        st = sv.iterate(4)
        return _bits(sv), sv.history(), sv.corrector_info(), st

    with ipm.IpmSolver(A, b, c, correctors=3) as sv:
        first = run(sv)
        again = run(sv)
        sch = sv.schedule()
    assert sch["blocks"] == 16 and sch["stream_at"] == 1 and sch["timeouts_recovered"] == 0, sch
    print("INFO overlapped", first[2])
    assert first[3]["iterations"] == 4 and first[2]["k"] == 3 and first[2]["rounds"] >= 4 and first[2]["accepted"] >= 1
    assert first[:3] == again[:3]
    monkeypatch.setenv("IPM_STREAM_AT", "0")
    with ipm.IpmSolver(A, b, c, correctors=3) as sv:
        single = run(sv)
        assert sv.schedule()["stream_at"] == 0
    assert single[:3] == first[:3]


# ---- the candidate vectors are written before they are read (the rule of tests/test_gpu_residue.py) ------------------------------
@pytest.mark.parametrize("name,as_sparse", [("dense/130x257b", False), ("sparse/129x16385", True)])
def test_rounds_do_not_depend_on_what_memory_held(name, as_sparse, monkeypatch):
    """mcc.mem (11 n-vectors, dy_g, the candidate's partial minima) is the library's own allocation, cleared whole on first use
    (rounds_ensure: the padding of v_g is read by the product with A).  Fresh handles with IPM_TEST_ALLOC_FILL = 0, 255 (NaN as doubles)
    and unset give the same bytes after iterate(3) with K = 3, rejected rounds included, and the 255 run is finite."""
    case = M.get(name)
    out = []
    for fill in ("0", "255", None):
        if fill is None:
            monkeypatch.delenv("IPM_TEST_ALLOC_FILL")
        else:
            monkeypatch.setenv("IPM_TEST_ALLOC_FILL", fill)
        with _solver(case, as_sparse=as_sparse, correctors=3) as sv:
            sv.set_state(*case.state())
            st = sv.iterate(3)
            assert st["iterations"] == 3 and sv.corrector_info()["rounds"] >= 3
            out.append((_bits(sv), sv.history(), sv.corrector_info()))
            if fill == "255":
                assert all(np.all(np.isfinite(v)) for v in sv.get_state())
    assert out[0] == out[1] == out[2]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_small_path_and_lockstep_handles_refuse_and_stay_usable():
    small = M.get("sparse/5x65b")
    with _solver(small, as_sparse=True) as sv:
        assert sv.schedule()["fused_small"] == 1
        with pytest.raises(_lib.IpmError, match="small"):
            sv.set_correctors(1)
        assert sv.correctors == 0 and sv.corrector_info()["k"] == 0
        sv.set_correctors(0)                                     # (k = 0 is accepted on every handle)
        sv.set_state(*small.state())
        assert sv.iterate(1)["iterations"] == 1
    with pytest.raises(_lib.IpmError, match="small"):
        _solver(small, as_sparse=True, correctors=1)
    lock = M.get("sparse/300x513")
    with _solver(lock, as_sparse=True, lockstep=True, factor="dense") as sv:
        with pytest.raises(_lib.IpmError, match="LOCKSTEP"):
            sv.set_correctors(1)
        sv.set_correctors(0)
        sv.set_state(*lock.state())
        assert ipm.lockstep_eligible(sv)
        with pytest.raises(ValueError, match="correctors"):
            ipm.solve_lockstep([sv], tol=1e-8, max_iter=2, correctors=1)
        st = ipm.solve_lockstep([sv], tol=1e-8, max_iter=2)
        assert st[0]["iterations"] == 2
    with pytest.raises(ValueError, match="correctors"):
        ipm.solve_small_batch([(sparse.csc_matrix(small.A), small.b, small.c)], correctors=1)
    with pytest.raises(ValueError, match="correctors"):
        ipm.IpmSolver(lock.A, lock.b, lock.c, correctors=_lib.MAX_CORRECTORS + 1)


def test_handle_moved_to_the_small_path_refuses_until_k_is_0():
    """The mirror of the last block of test_gpu_refine.test_refusals, with its 128 x 600 pair (ipm_set_A_csc decides the path: 600 dense
    columns of 128 rows are past the product-list cap of the one-workgroup kernel, the sparse matrix of the same shape is not): a
    handle that went onto the small path after K > 0 is refused by the solve entries until set_correctors(0), which it accepts."""
    rng = np.random.default_rng(3)
    m, n = 128, 600
    Ab = rng.standard_normal((m, n))
    Ab[:, :m] += 4.0 * np.eye(m)
    cols = np.arange(m, n)
    Asm = sparse.csc_matrix((np.ones(m + 2 * cols.size), (np.concatenate([np.arange(m), cols % m, (7 * cols + 1) % m]),
                                                          np.concatenate([np.arange(m), cols, cols]))), shape=(m, n))
    Asm.sort_indices()
    with ipm.IpmSolver(sparse.csc_matrix(Ab), Ab @ np.ones(n), np.ones(n), reorder=None, correctors=1) as sv:
        assert sv.schedule()["fused_small"] == 0 and sv._perm is None
        indptr, indices, data = Asm.indptr.astype(np.int32), Asm.indices.astype(np.int32), Asm.data.astype(np.float64)
        sv._check(sv._lib.ipm_set_A_csc(sv._h, indptr.ctypes.data_as(C.POINTER(C.c_int32)), indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                        data.ctypes.data_as(C.POINTER(C.c_double)), int(data.shape[0])))
        assert sv.schedule()["fused_small"] == 1 and sv.corrector_info()["k"] == 1
        sv.init_state(1.0)
        for call in (lambda: sv.iterate(1), lambda: sv.solve(max_iter=2)):
            with pytest.raises(_lib.IpmError, match="small"):
                call()
        sv.set_correctors(0)
        assert sv.correctors == 0 and sv.corrector_info()["k"] == 0
        assert sv.iterate(1)["iterations"] == 1


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _load_general(name):
    z = np.load(os.path.join(GOLDEN, "general", name + ".npz"))

    def mat(p):
        if p + "_none" in z.files or p + "_data" not in z.files:
            return None
        return sparse.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(int(v) for v in z[p + "_shape"]))

    return dict(c=z["c"], Aeq=mat("Aeq"), beq=z["beq"] if "beq" in z.files else None, Aineq=mat("Aineq"),
                bineq=z["bineq"] if "bineq" in z.files else None, lb=z["lb"], ub=z["ub"])


def _e2e_lp(which):
    if which == "dense_syn_256x512":
        z = np.load(os.path.join(GOLDEN, "dense_syn_256x512.npz"))
        A, _, _ = synthetic_lp(256, 512)
        return A, z["b"].ravel(), z["c"].ravel(), None, dict(y0=0.0)
    F = G.native_form(**_load_general("GROW22"))
    return F.A, np.asarray(F.b).ravel(), np.asarray(F.c).ravel(), F.u, dict(start="mehrotra")


def _stop_quantities(A, b, c, u, x, y, s, w, z):
    """rp, rd, gap and the norms of the stop test (stop_test_kernel_body), in longdouble."""
    L = IO.LD
    x, y, s, w, z, b, c = (np.asarray(v, dtype=L).ravel() for v in (x, y, s, w, z, b, c))
    U = np.isfinite(u)
    uu = np.where(U, u, 0.0).astype(L)
    ax = np.asarray(A @ np.asarray(x, dtype=np.float64), dtype=L) if sparse.issparse(A) else A.astype(L) @ x
    aty = np.asarray(A.T @ np.asarray(y, dtype=np.float64), dtype=L) if sparse.issparse(A) else A.T.astype(L) @ y
    ru = np.where(U, x + w - uu, L(0))
    rp = np.sqrt(((ax - b) ** 2).sum() + (ru ** 2).sum())
    rd = IO.norm(aty + s - z - c)
    return dict(rp=rp, rd=rd, gap=x @ s + w @ z, bn=np.sqrt(b @ b + uu @ uu), cn=IO.norm(c), xn=IO.norm(x),
                yzn=np.sqrt(y @ y + z @ z))


E2E_TOL = 1e-8


@pytest.mark.parametrize("which", ["dense_syn_256x512", "GROW22"])
@pytest.mark.parametrize("eta", [0.91, 0.995])
def test_end_to_end_with_two_rounds(which, eta):
    A, b, c, u, kw = _e2e_lp(which)
    n = c.shape[0]
    uvec = np.full(n, np.inf) if u is None else np.asarray(u, dtype=np.float64)
    runs = {}
    for K in (0, 2):
        x, y, s, info = ipm.solve_with_info(A, b, c, ub=u, tol=E2E_TOL, max_iter=500, eta=eta, correctors=K, **kw)
        w, z = (info["w"], info["z"]) if info["bounded"] else (np.zeros(n), np.zeros(n))
        q = _stop_quantities(A, b, c, uvec, x, y, s, w, z)
        print("ITERS %s eta=%g K=%d iterations=%d correctors=%s objective=%.15e" % (which, eta, K, info["iterations"], info["correctors"],
                                                                                     info["objective"]))
        print("STOP %s eta=%g K=%d rp/(1+bn)=%.3e rd/(1+cn)=%.3e gap=%.3e" % (which, eta, K, float(q["rp"] / (1 + q["bn"])),
                                                                               float(q["rd"] / (1 + q["cn"])), float(q["gap"])))
        assert info["status"] == 1 and info["correctors"]["k"] == K, info
        if K:
            assert info["correctors"]["rounds"] >= 1
        else:
            assert info["correctors"] == dict(k=0, rounds=0, accepted=0, iterations=0)
        assert q["rp"] <= E2E_TOL * (1 + q["bn"]) and q["rd"] <= E2E_TOL * (1 + q["cn"]) and q["gap"] <= E2E_TOL, (which, eta, K)
        assert np.all(x > 0) and np.all(s > 0)
        runs[K] = (info["objective"], q)
    q0, q2 = runs[0][1], runs[2][1]
    bound = E2E_TOL + 2 * E2E_TOL * (1 + q0["bn"]) * max(q0["yzn"], q2["yzn"]) + 2 * E2E_TOL * (1 + q0["cn"]) * max(q0["xn"], q2["xn"])
    diff = abs(runs[0][0] - runs[2][0])
    print("OBJ %s eta=%g |difference| %.3e bound %.3e" % (which, eta, diff, float(bound)))
    assert diff <= bound
