"""No kernel may read or write outside the memory it was given.

test_gpu_residue.py closed one half of a class of silent error (a result that depends on what device memory held before); this file
closes the other: an overrun.  The workspace packs twenty regions back to back, everything else comes from a pool whose blocks are
reused on purpose, and the Python front end allocates the workspace exactly -- an overrun lands in the next region or the next
block, is usually overwritten before anyone reads it, and the numbers still come out right.  With IPM_TEST_ALLOC_GUARD set
(csrc/host_handle.h; tests/guard_bands.py) every allocation of the library lies between two bands of 131072 bytes -- one
128 x 128 tile of doubles -- filled with a band byte, and the workspace has one band before its first region, between every two
regions and behind the last.

Every cell builds fresh handles three times: knob unset, guarded with band byte 0xFF, guarded with 0x00 (a stray 0.0 is invisible
in a 0x00 band, a stray NaN / -1 in a 0xFF one), and asserts, with no tolerance anywhere:
  1. in both guarded runs every live band of the process is intact after EACH operation (guard_bands.Checked compares after every
     method call of a solver; batches and the handle-less LU calls compare explicitly), nothing guarded is left alive once the
     handles are closed, and the violation log (what dev_free / ipm_destroy found when they compared before releasing) is empty;
  2. the observables -- test_gpu_residue._observe: form_normal_matrix over 12 decades, both Newton directions with their scalars,
     get_factor, the state after iterate(3), and after solve() its statistics without solve_ms, history() and the state -- are
     bytewise equal between the three runs: 0xFF against 0x00 shows that no value read from outside an allocation reaches a
     result, unset against guarded that the guard changes nothing;
  3. the cell took the path it names (schedule() / factor_info() / corrector_info() / refine_info() / dense_split_info()).

THE PADDING RULE (part 4).  ipm_create zeroes everything behind A and B "because padding entries of every vector must stay 0"; the
GEMVs and the two-level reductions run over padded lengths and rely on it.  In the guarded runs the tails [n, np) of the eleven
n-vectors and [m, mp) of the seven m-vectors are read back after every iterate() and solve() of a solver whose workspace is a torch
tensor (guard_bands.tails, through the listing's addresses) and must be zero bytes, with ONE audited exception (TAIL_EXCEPTIONS):
  vector  tail holds          written by                                                      read by, and why it is harmless
  ------  ------------------  --------------------------------------------------------------  ------------------------------------------
  t1      -0.0 (the sign bit  gemv_n_kernel / spmv_csr_kernel (vector_ops.h, sparse_ops.h):   the substitutions of enqueue_normal_solve
          only) wherever      the right-hand side -r_b - A v is out[row] = sa * s + sb *      and the refinement's residual, over mp rows:
          mp > m              add[row] for every row < mp with sa = sb = -1; on a padding     they only multiply and add it, and rows >= m
                              row s = +0 (A's padding rows are zero) and add = r_b's tail =   of L are identity rows, so the entry is an
                              +0, and (-1)(+0) + (-1)(+0) = -0.0.  The lockstep twins are     exact zero in every sum it enters; dy's and
                              the same bodies; the one-workgroup kernel keeps its rhs in      dya's tails, which those solves write, read
                              LDS (t1s, rows >= m set to 0), so on a small-path handle only   back as zero bytes in every cell.
                              the seams (ipm_newton_direction) leave the -0.0.
  The value is a zero, so this is no bug; the test does not drop t1 but pins its tail to zero BY VALUE (a NaN, a denormal or any
  other number there fails).  The other seventeen tails are zero bytes after every iterate() and solve() of every cell.

CELLS (each the smallest shape that reaches its path; once with padding and once without slack where the path allows both)
  dense multi-kernel          1x1, 128x256 (no slack), 130x257, 130x257 bounded
  ragged groups               9 blocks: 1100x1400 and 1152x1408 (no slack); default, block steps, two-level
  fused formation + factor    forced, 384x640 (3 blocks exact) and 385x600 (3 blocks + 1 row), IPM_STREAM_AT 1 and 0 (below 16 blocks no
                              residual stream exists: the schedule word is 0 either way, asserted); the streamed A^T dy itself at
                              2048x2500 (16 blocks exact) with IPM_STREAM_AT 1 and 0
  small path                  5x65b and AFIRO, IPM_FUSED_SMALL 1 and 0
  sparse ingest, dense factor 130x257b and 256x512 (no slack) with IPM_LIST_FORM 1 and 0; block-bidiagonal 500 rows with IPM_ENVELOPE 1 and 0
  sparse factor               path300, star106, bigborder_300_20 in both IPM_SP_MODEs
  batches                     lockstep with a late join; lockstep with bounds; small batch; small QP batch; small free batch
  device LU                   n = 64, 65, 128, 129 with IPM_LU_NB unset and 128, 9 right-hand sides
  features                    quadratic term (multi-kernel; small with quad_small); free columns with curvature (multi-kernel;
                              free_small); LP free columns plain and bounded; infeasibility detection LP and QP ending in status 5
                              and 6 with the certificate read; correctors k = 2; refinement k = 2; the dense-column split;
                              ipm_equilibrate dense and sparse with the device Mehrotra start on the multi-kernel and small paths
  re-setters                  ipm_set_A_* a second time with fewer nonzeros (sparse, dense); set-then-clear of the quadratic term, the
                              bounds and both free sets
  controls                    a planted byte in a workspace band (between two regions, behind the last) and in a pool block's band
                              (bnd_mem) is reported at exactly that band, side and offset; restored, the handle still solves; planted
                              again and left, the release logs it
Cells dropped: none.  FINDINGS: no band was damaged and no result differed between the three runs in any cell; the one nonzero tail
is the audited -0.0 of t1.  The file runs in about 14 seconds on an MI355X.

WHICH CELL FAILS WHEN THE INSTRUMENT IS REVERTED (run once on an MI355X with three libraries built from host code with that part taken
out, profiles/alloc_guard_reversion_check.txt): without the band fill in dev_malloc, all of test_dense_multi_kernel (the bands of
d_flags, bnd_mem, ... hold what the pool block held: damage at the first comparison) and test_control_pool_block; without the gaps
in make_layout, test_control_workspace (no band between two regions to plant in), test_dense_multi_kernel (a guarded solver
carries no workspace bands) and tests/test_alloc_guard_host.py; without the comparison in dev_free, test_control_pool_block (the
byte left in bnd_mem's band must be in the log after close).
"""
import ctypes as C
import re

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib
from interiorpointmethod_amd.workloads import synthetic_lp

import dense_split_cases as DC
import guard_bands as GB
import infeas_cases as IC
import iteration_oracle as IO
import qp_infeas_cases as QC
import sparse_cases as SC
import test_gpu_residue as RES
from test_gpu_residue import Obs, _observe

pytestmark = pytest.mark.gpu

# name of an n- or m-vector -> why its padding tail may hold bytes other than zero (the audit is in the docstring).  An exception is
# as narrow as its reading allows: t1's tail must still be ZERO BY VALUE (+0.0 or -0.0), every other tail zero bytes.
TAIL_EXCEPTIONS = {"t1": "-0.0: gemv_n_kernel / spmv_csr_kernel write -1 * (+0) + -1 * (+0) on the padding rows"}


class Run:
    """One of the three runs of a cell."""

    def __init__(self, byte):
        self.byte, self.guarded, self.tail_findings = byte, byte is not None, []

    def check(self, where=""):
        if self.guarded:
            GB.assert_intact(None, where)
        else:
            assert _lib.guard_list() == []

    def after(self, sv, name):
        self.check("after %s on %d x %d" % (name, sv.m, sv.n))
        if self.guarded and name in ("iterate", "solve") and sv._ws is not None:
            self.tails(sv, name)

    def tails(self, sv, name):
        bad = [nm for nm, raw in sorted(GB.tails(sv).items()) if any(raw) and not (nm in TAIL_EXCEPTIONS and not np.any(np.frombuffer(raw)))]
        if bad:
            self.tail_findings.append((name, sv.m, sv.n, bad))

    def solver(self, *a, **kw):
        """A solver built under this run's knob; guarded, it must really carry bands (the workspace's 21 at least)."""
        sv = ipm.IpmSolver(*a, **kw)
        n = len(sv.guard_bands())
        assert (n >= 21) if self.guarded else (n == 0), n
        return GB.Checked(sv, self.after)


def _three(monkeypatch, run, env=None, ran=True):
    """run(G) -> Obs on fresh handles, with the knob unset, guarded 0xFF and guarded 0x00; the comparisons of a cell."""
    res = {}
    _lib.guard_log()                                            # (what an earlier, failed cell may have left)
    for byte in (None,) + GB.BYTES:
        with monkeypatch.context() as mp:
            for k, v in (env or {}).items():
                mp.setenv(k, v)
            with GB.guard(mp, byte):
                G = Run(byte)
                res[byte] = run(G)
                G.check("at the end of the run")
            GB.assert_released("(band byte %r)" % byte)
            assert not G.tail_findings, ("nonzero padding tails (band byte %r)" % byte, G.tail_findings)
    unset, ff, zero = res[None], res[0xFF], res[0x00]
    assert sorted(unset.bytes) == sorted(ff.bytes) == sorted(zero.bytes)
    differ = [k for k in sorted(ff.bytes) if ff.bytes[k] != zero.bytes[k]]
    assert not differ, ("band byte 0xFF against 0x00: a value from outside an allocation reaches a result", differ)
    differ = [k for k in sorted(ff.bytes) if ff.bytes[k] != unset.bytes[k]]
    assert not differ, ("knob unset against guarded", differ)
    if ran:
        RES._ran(unset)
    return unset


def _lp(m, n, seed, free=(), density=None):
    """A strictly feasible primal-dual pair: b = A x0, c = A^T y0 + s0 with x0, s0 > 0; on the `free` columns x0 has any sign and s0 = 0."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    if density is not None:
        A *= rng.random((m, n)) < density
        A[np.arange(m), rng.integers(0, n, m)] = 1.0 + rng.random(m)            # no empty row
    x0, s0, y0 = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), rng.standard_normal(m)
    free = np.asarray(list(free), dtype=int)
    x0[free], s0[free] = rng.standard_normal(free.size), 0.0
    return A, A @ x0, A.T @ y0 + s0


# ---- dense ingest, multi-kernel path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,bounded", [(1, 1, False), (128, 256, False), (130, 257, False), (130, 257, True)], ids=["1x1", "128x256", "130x257", "130x257b"])
def test_dense_multi_kernel(monkeypatch, m, n, bounded):
    A, b, c = synthetic_lp(m, n, seed=11)
    ub = RES._half_bounded(n) if bounded else None

    def run(G):
        with G.solver(A, b, c, ub=ub) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert not sv.sparse and sv.factor == "dense" and sch["fused_small"] == 0 and sch["fused_factor"] == 0, sch
            assert sch["blocks"] == (m + 127) // 128 and sv.bounded == (0 if ub is None else int(np.isfinite(ub).sum()))
            assert sch["grouped_trsv"] == (1 if m > 128 else 0), sch
        return o
    _three(monkeypatch, run)


@pytest.mark.parametrize("shape", [(1100, 1400), (1152, 1408)], ids=["1100x1400", "1152x1408"])
@pytest.mark.parametrize("variant", sorted(RES.RAGGED))
def test_ragged_groups(monkeypatch, variant, shape):
    env, want = RES.RAGGED[variant]
    A, b, c = synthetic_lp(*shape, seed=12)

    def run(G):
        with G.solver(A, b, c) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sch["blocks"] == 9 and sch["fused_factor"] == 0 and sch["fused_small"] == 0, sch
            assert {k: sch[k] for k in want} == want, sch
        return o
    _three(monkeypatch, run, env)


# ---- fused formation + factorization, streamed A^T dy ----------------------------------------------------------------------
@pytest.mark.parametrize("stream_at", [1, 0])
@pytest.mark.parametrize("shape,blocks", [((384, 640), 3), ((385, 600), 4)], ids=["3-blocks-exact", "3-blocks+1-row"])
def test_fused_formation_and_factorization(monkeypatch, shape, blocks, stream_at):
    A, b, c = synthetic_lp(*shape, seed=13)

    def run(G):
        with G.solver(A, b, c) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sch["blocks"] == blocks and sch["fused_factor"] == 1 and sch["device_polling"] == 1, sch
            assert sch["stream_at"] == 0, sch                  # (no residual stream below 16 blocks, whatever the switch says)
        return o
    _three(monkeypatch, run, {"IPM_FUSED_FACTOR": "force", "IPM_STREAM_AT": str(stream_at)})


@pytest.mark.parametrize("stream_at", [1, 0])
def test_streamed_at(monkeypatch, stream_at):
    A, b, c = synthetic_lp(2048, 2500, seed=7)

    def run(G):
        with G.solver(A, b, c) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sch["blocks"] == 16 and sch["stream_at"] == stream_at and sch["grouped_trsv"] == 1, sch
        return o
    _three(monkeypatch, run, {} if stream_at else {"IPM_STREAM_AT": "0"})


# ---- the one-workgroup small path and its multi-kernel twin ----------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["5x65b", "AFIRO"])
def test_small_path(monkeypatch, name, fused):
    A, b, c, ub = RES._small_lp(name)

    def run(G):
        with G.solver(A, b, c, ub=ub) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sv.sparse and sv.factor == "dense" and sch["fused_small"] == fused and sch["blocks"] == 1, sch
            assert sv.bounded == (0 if ub is None else int(np.isfinite(ub).sum()))
        return o
    _three(monkeypatch, run, {} if fused else {"IPM_FUSED_SMALL": "0"})


# ---- sparse A, dense factor ------------------------------------------------------------------------------------------------
def _sparse_case(name):
    if name == "130x257b":
        A, b, c, ub = RES._feasible(IO.get("sparse/" + IO.shape_name(*IO.SMALL, True)))
        return sparse.csc_matrix(A), b, c, ub, 2
    A, b, c = _lp(256, 512, 21, density=0.06)                                 # 256 x 512: two blocks, no padding row or column
    return sparse.csc_matrix(A), b, c, None, 2


@pytest.mark.parametrize("list_form", [1, 0])
@pytest.mark.parametrize("name", ["130x257b", "256x512"])
def test_sparse_ingest_dense_factor(monkeypatch, name, list_form):
    A, b, c, ub, blocks = _sparse_case(name)

    def run(G):
        with G.solver(A, b, c, ub=ub, factor="dense") as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sv.sparse and sv.factor == "dense" and sch["fused_small"] == 0 and sch["blocks"] == blocks, sch
        return o
    _three(monkeypatch, run, {} if list_form else {"IPM_LIST_FORM": "0"})


@pytest.mark.parametrize("envelope", [1, 0])
def test_tiles_outside_the_envelope(monkeypatch, envelope):
    A, b, c = RES._block_bidiagonal()

    def run(G):
        with G.solver(A, b, c, factor="dense", reorder=None) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sv.sparse and sch["blocks"] == 4 and sch["envelope"] == envelope and sch["fused_small"] == 0, sch
        return o
    _three(monkeypatch, run, {} if envelope else {"IPM_ENVELOPE": "0"})


# ---- the sparse factor -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["task", "level"])
@pytest.mark.parametrize("name", ["path300", "star106", "bigborder_300_20"])
def test_sparse_factor(monkeypatch, name, mode):
    A, b, c, ub = RES._feasible(SC.iteration_case(name, False))
    A = sparse.csc_matrix(A)
    rng = np.random.default_rng(3)
    M = rng.standard_normal((A.shape[0], A.shape[0] + 7))
    spd, rhs = M @ M.T + np.eye(A.shape[0]), rng.standard_normal(A.shape[0])
    t = SC.tree(name)
    for k in RES.SP_ENV:
        monkeypatch.delenv(k, raising=False)

    def run(G):
        with G.solver(A, b, c, ub=ub, factor="sparse") as sv:
            fi = sv.factor_info()
            assert sv.factor == "sparse" and (fi["panels"], fi["height"], fi["widest_front"]) == (t.nsn, t.height, t.rmax), fi
            o = Obs()
            sv.init_state(0.0)
            o.put("first.affine", sv.newton_direction(False))              # before any dense entry point: no B_own yet
            o.put("solve_linear", sv.solve_linear(spd, rhs))               # allocates B_own and invD_own
            _observe(sv, o)
            sch = RES._clean(sv)
            assert sch["sparse_level_mode"] == (1 if mode == "level" else 0) and sv.factor_info()["serial_launches"] == 0, sch
        return o
    _three(monkeypatch, run, {"IPM_SP_MODE": mode})


# ---- batches ---------------------------------------------------------------------------------------------------------------
def _lockstep(G, make, late):
    """The solvers of make() in one lockstep batch, the last `late` of them joining between two steps."""
    svs = make()
    try:
        for sv in svs:
            assert ipm.lockstep_eligible(sv._sv)
            sv.init_state(1.0)
        done = []
        with ipm.LockstepBatch(tol=1e-8, max_iter=40) as bt:
            for sv in svs[:len(svs) - late]:
                bt.add(sv._sv)
            done += bt.step()
            G.check("after the first lockstep step")
            for sv in svs[len(svs) - late:]:
                bt.add(sv._sv)
            for _ in range(60):
                if not bt.active:
                    break
                done += bt.step()
                G.check("after a lockstep step")
            assert bt.active == 0 and sorted(id(s) for s in done) == sorted(id(s._sv) for s in svs)
        G.check("after the batch is closed")
        o = Obs()
        for i, sv in enumerate(svs):
            o.solves.append((sv.stats["status"], sv.stats["iterations"]))
            o.put("lp%d.stats" % i, sv.stats)
            o.put("lp%d.state" % i, sv.get_state())
            o.put("lp%d.bound_state" % i, sv.get_bound_state())
            o.put("lp%d.history" % i, sv.history())
            assert sv.schedule()["timeouts_recovered"] == 0
            if G.guarded:
                G.tails(sv._sv, "lockstep batch")
    finally:
        for sv in svs:
            sv.close()
    return o


def test_lockstep_batch_with_a_late_join(monkeypatch):
    probs = [IC.netlib(nm) for nm in ("SC205", "E226", "BANDM")]

    def run(G):
        def make():
            svs = [G.solver(*p, lockstep=True, factor="dense") for p in probs]
            assert [sv.schedule()["blocks"] for sv in svs] == [2, 2, 3]
            return svs
        return _lockstep(G, make, late=1)
    _three(monkeypatch, run)


def test_lockstep_batch_with_bounds(monkeypatch):
    A, b, c, ub = RES._feasible(IO.get("sparse/" + IO.shape_name(*IO.SMALL, True)))
    A = sparse.csc_matrix(A)
    plain = IC.netlib("SC205")

    def run(G):
        def make():
            svs = [G.solver(A, b, c, ub=ub, lockstep=True, lockstep_bounds=True, factor="dense"), G.solver(*plain, lockstep=True, factor="dense"),
                   G.solver(A, b, c, ub=ub, lockstep=True, lockstep_bounds=True, factor="dense")]
            assert svs[0].bounded == int(np.isfinite(ub).sum()) > 0 and svs[1].bounded == 0
            return svs
        return _lockstep(G, make, late=1)
    _three(monkeypatch, run)


def _small_batch(G, make, max_iter=100, mehrotra=False):
    svs = make()
    try:
        assert all(sv.schedule()["fused_small"] == 1 for sv in svs)
        raw = [sv._sv for sv in svs]
        o = Obs()
        if mehrotra:
            o.put("start.pivots_fixed", ipm.init_small_batch_mehrotra(raw))
            G.check("after the batched Mehrotra start")
            for i, sv in enumerate(svs):
                o.put("lp%d.start" % i, sv.get_state())
        else:
            for sv in svs:
                sv.init_state(1.0)
        stats = ipm.solve_small_batch_solvers(raw, tol=1e-8, max_iter=max_iter)
        G.check("after the small batch")
        for i, (sv, st) in enumerate(zip(svs, stats)):
            o.solves.append((st["status"], st["iterations"]))
            o.put("lp%d.stats" % i, st)
            o.put("lp%d.state" % i, sv.get_state())
            o.put("lp%d.bound_state" % i, sv.get_bound_state())
            o.put("lp%d.history" % i, sv.history())
            if G.guarded:
                G.tails(sv._sv, "small batch")
    finally:
        for sv in svs:
            sv.close()
    return o


def _half(n, value):
    return np.where(np.arange(n) % 2 == 0, value, np.inf)


def test_small_batch(monkeypatch):
    probs = [IC.netlib(nm) for nm in ("AFIRO", "SC50A", "KB2", "ADLITTLE")]
    opts = [dict(), dict(scale="ruiz"), dict(ub=1e3), dict(scale="ruiz", ub=1e3)]

    def run(G):
        def make():
            return [G.solver(A, b, c, **dict(kw, **({"ub": _half(A.shape[1], kw["ub"])} if "ub" in kw else {}))) for (A, b, c), kw in zip(probs, opts)]
        return _small_batch(G, make, mehrotra=True)
    _three(monkeypatch, run)


def _g(n, seed, every=2):
    return np.where(np.arange(n) % every == 0, np.random.default_rng(seed).uniform(0.1, 2.0, n), 0.0)


def test_small_qp_batch(monkeypatch):
    probs = [IC.netlib(nm) for nm in ("AFIRO", "SC50A", "KB2")]

    def run(G):
        def make():
            svs = [G.solver(A, b, c, quad=_g(A.shape[1], i), quad_small=True, **({"ub": _half(A.shape[1], 1e3)} if i == 2 else {}))
                   for i, (A, b, c) in enumerate(probs)]
            assert all(sv.quadratic_nonzeros() > 0 for sv in svs)
            return svs
        return _small_batch(G, make)
    _three(monkeypatch, run)


def _free_small_problem(seed, m=20, n=60, k=5, bounded=False):
    free = np.arange(0, 4 * k, 4)
    A, b, c = _lp(m, n, seed, free=free, density=0.3)
    g = _g(n, seed, every=4)                                                   # curvature exactly on the free columns' residue class
    ub = None
    if bounded:
        ub = np.full(n, np.inf)
        ub[1::4] = 3.0                                                           # above every x0, never on a free column
    return sparse.csc_matrix(A), b, c, g, free, ub


def test_small_free_batch(monkeypatch):
    probs = [_free_small_problem(31), _free_small_problem(32, m=27, n=70, k=6, bounded=True)]

    def run(G):
        def make():
            svs = [G.solver(A, b, c, quad=g, free=free, ub=ub, free_small=True) for A, b, c, g, free, ub in probs]
            assert all(len(sv.free_columns()) > 0 for sv in svs)
            return svs
        return _small_batch(G, make)
    _three(monkeypatch, run)


# ---- device LU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [None, "128"])
@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_device_lu(monkeypatch, n, nb):
    k, lda, ldb, ldx = 9, n + 7, 12, 11
    rng = np.random.default_rng(n)
    A = np.zeros((n, lda)); A[:, :n] = rng.standard_normal((n, n)); A[np.arange(n), rng.permutation(n)] += 2.0 * np.sqrt(n)
    B = np.zeros((n, ldb)); B[:, :k] = rng.standard_normal((n, k))
    PD, lib = C.POINTER(C.c_double), _lib.load()

    def run(G):
        X, LU, piv, info = np.zeros((n, ldx)), np.zeros((n, lda)), np.zeros(n, dtype=np.int32), C.c_int64(-1)
        rc = lib.ipm_lu_solve(0, n, A.ctypes.data_as(PD), lda, k, B.ctypes.data_as(PD), ldb, X.ctypes.data_as(PD), ldx, C.byref(info))
        assert rc == _lib.IPM_OK and info.value == 0, (rc, info.value)
        GB.assert_released("after ipm_lu_solve")            # the call owns its memory: every block was compared when it was freed
        rc = lib.ipm_lu_factor(0, n, A.ctypes.data_as(PD), lda, LU.ctypes.data_as(PD), lda, piv.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info))
        assert rc == _lib.IPM_OK and info.value == 0, (rc, info.value)
        GB.assert_released("after ipm_lu_factor")
        o = Obs()
        o.put("X", X[:, :k]); o.put("LU", LU[:, :n]); o.put("piv", piv)
        assert not np.any(X[:, k:]) and not np.any(LU[:, n:])
        return o
    o = _three(monkeypatch, run, {} if nb is None else {"IPM_LU_NB": nb}, ran=False)
    X = np.frombuffer(o.bytes["X"]).reshape(n, k)
    assert np.linalg.norm(A[:, :n] @ X - B[:, :k]) <= 1e-10 * np.linalg.norm(B[:, :k])


# ---- features --------------------------------------------------------------------------------------------------------------
FEATURES = {}          # cell -> (constructor keywords from (m, n), the path assertion on the solver after _observe)


def _feature(name):
    def deco(f):
        FEATURES[name] = f
        return f
    return deco


@_feature("quad")
def _():
    A, b, c = _lp(130, 257, 41)
    return (A, b, c), dict(quad=_g(257, 41)), lambda sv, sch: sv.quadratic_nonzeros() == 129 and sch["fused_small"] == 0 and sch["blocks"] == 2


@_feature("quad-no-slack")
def _():
    A, b, c = _lp(128, 256, 42)
    return (A, b, c), dict(quad=_g(256, 42), ub=_half(256, 3.0)), lambda sv, sch: sv.quadratic_nonzeros() == 128 and sv.bounded == 128 and sch["blocks"] == 1


@_feature("quad-small")
def _():
    A, b, c = IC.netlib("AFIRO")
    return (A, b, c), dict(quad=_g(A.shape[1], 43), quad_small=True), lambda sv, sch: sv.quadratic_nonzeros() > 0 and sch["fused_small"] == 1


@_feature("free")
def _():
    free = np.arange(0, 257, 8)
    A, b, c = _lp(130, 257, 44, free=free)
    return (A, b, c), dict(quad=_g(257, 44, every=4), free=free), lambda sv, sch: len(sv.free_columns()) == 33 and sch["fused_small"] == 0 and sch["blocks"] == 2


@_feature("free-bounded-no-slack")
def _():
    free = np.arange(0, 256, 8)
    A, b, c = _lp(128, 256, 45, free=free)
    ub = np.full(256, np.inf)
    ub[1::4] = 3.0
    return (A, b, c), dict(quad=_g(256, 45, every=4), free=free, ub=ub), lambda sv, sch: len(sv.free_columns()) == 32 and sv.bounded == 64


@_feature("free-small")
def _():
    A, b, c, g, free, ub = _free_small_problem(46)
    return (A, b, c), dict(quad=g, free=free, free_small=True), lambda sv, sch: len(sv.free_columns()) == 5 and sch["fused_small"] == 1


@_feature("free-lp")
def _():
    free = np.arange(3, 257, 16)
    A, b, c = _lp(130, 257, 47, free=free)
    return (A, b, c), dict(free_lp=free), lambda sv, sch: len(sv.free_lp_columns()[0]) == 16 and sch["blocks"] == 2


@_feature("free-lp-bounded-no-slack")
def _():
    free = np.arange(3, 256, 16)
    A, b, c = _lp(128, 256, 48, free=free)
    return (A, b, c), dict(free_lp=free, ub=_half(256, 3.0)), lambda sv, sch: len(sv.free_lp_columns()[0]) == 16 and sv.bounded == 128


@_feature("correctors")
def _():
    return synthetic_lp(130, 257, seed=49), dict(correctors=2), lambda sv, sch: sv.corrector_info()["k"] == 2 and sv.corrector_info()["rounds"] > 0


@_feature("refine")
def _():
    return synthetic_lp(130, 257, seed=50), dict(refine=2), lambda sv, sch: sv.refine_info().k == 2 and sv.refine_info()[1] > 0


@_feature("refine-bounded-no-slack")
def _():
    return synthetic_lp(128, 256, seed=51), dict(refine=2, correctors=2, ub=_half(256, 3.0)), \
        lambda sv, sch: sv.refine_info().k == 2 and sv.corrector_info()["k"] == 2 and sv.bounded == 128


@_feature("dense-split")
def _():
    A, cols = DC.arrowhead(m=150, k=3, block=50, seed=3)
    n = A.shape[1]
    return (A, np.asarray(A @ np.ones(n)).ravel(), np.ones(n)), dict(factor="sparse", dense_cols=cols), \
        lambda sv, sch: sv.factor == "sparse" and sv.dense_split_info()["k"] == 3 and sv.dense_split_info()["factorizations"] > 0


@pytest.mark.parametrize("cell", sorted(FEATURES))
def test_feature(monkeypatch, cell):
    (A, b, c), kw, took = FEATURES[cell]()

    def run(G):
        with G.solver(A, b, c, **kw) as sv:
            o = _observe(sv)
            sch = RES._clean(sv)
            assert took(sv, sch), (cell, sch)
        return o
    _three(monkeypatch, run)


@pytest.mark.parametrize("path", ["multi-kernel", "multi-kernel-no-slack", "small", "sparse"])
def test_equilibrate_and_mehrotra_start(monkeypatch, path):
    """ipm_equilibrate on a dense and on a sparse handle, then the device Mehrotra start."""
    if path == "small":
        A, b, c = IC.netlib("AFIRO")
    else:
        m, n = (128, 256) if path == "multi-kernel-no-slack" else (130, 257)
        A, b, c = synthetic_lp(m, n, seed=14)
        A = A * 2.0 ** np.random.default_rng(1).integers(-12, 13, (m, 1))      # rows over 24 binades: the passes have work to do
        if path == "sparse":
            A = sparse.csc_matrix(A * (np.random.default_rng(2).random((m, n)) < 0.2) + np.eye(m, n))
    kw = dict(factor="dense") if path == "sparse" else {}

    def run(G):
        with G.solver(A, b, c, scale="ruiz", **kw) as sv:
            o = Obs()
            assert sv.scale_info["passes"] >= 1
            o.put("scaling", sv.scaling()[:2])
            o.put("start.pivots_fixed", sv.init_state_mehrotra())
            o.put("start.state", sv.get_state())
            o.put("iterate3.stats", sv.iterate(3))
            o.put("iterate3.state", sv.get_state())
            o.put("history", sv.history())
            sch = RES._clean(sv)
            assert sv.sparse == (path in ("small", "sparse")) and sch["fused_small"] == (1 if path == "small" else 0), sch
            assert sch["blocks"] == (1 if path in ("small", "multi-kernel-no-slack") else 2), sch
        return o
    _three(monkeypatch, run, ran=False)


DETECT = {"lp-primal": lambda: dict(IC.small_instances()["primal_dense"](), g=None, free=None),
          "lp-dual": lambda: dict(IC.small_instances()["dual_dense"](), g=None, free=None),
          "lp-bounded-primal": lambda: dict(IC.bounded_primal_infeasible(), g=None, free=None),
          "qp-primal": QC.sep_primal, "qp-bounded-primal": QC.sep_bounded_primal, "qp-dual": QC.sep_dual,
          "qp-factor-primal": QC.factor_primal, "qp-factor-dual": QC.factor_dual}


@pytest.mark.parametrize("cell", sorted(DETECT))
def test_infeasibility_certificate(monkeypatch, cell):
    """cert_mem is 2 n + m doubles, unpadded, and certificate_kernel runs a grid over max(n, m)."""
    P = DETECT[cell]()
    kw = dict(detect_infeasibility=True) if P["g"] is None else dict(detect_qp=True, quad=P["g"], free=P.get("free"))

    def run(G):
        with G.solver(P["A"], P["b"], P["c"], ub=P.get("ub"), **kw) as sv:
            sv.init_state(1.0)
            st = sv.solve(tol=1e-8, max_iter=200)
            assert st["status"] == IC.KIND[P["kind"]], st
            o = Obs()
            o.put("stats", st)
            cert = sv.certificate()
            assert cert["kind"] == P["kind"] and cert["k"] == st["iterations"]
            o.put("certificate", cert)
            o.put("history", sv.history())
            o.put("state", sv.get_state())
            RES._clean(sv)
        return o
    _three(monkeypatch, run, ran=False)


# ---- re-setters: they free and reallocate --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_a_second_A_with_fewer_nonzeros(monkeypatch, kind):
    A1, A2, b, c, ub = RES._second_A(kind)
    kw = dict(factor="dense", reorder=None) if kind == "sparse" else {}
    PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def run(G):
        with G.solver(A1, b, c, ub=ub, **kw) as sv:
            _observe(sv, max_iter=5)
            if kind == "sparse":
                ip, ix, v = A2.indptr.astype(np.int32), A2.indices.astype(np.int32), A2.data.astype(np.float64)
                rc = sv._lib.ipm_set_A_csc(sv._h, ip.ctypes.data_as(PI), ix.ctypes.data_as(PI), v.ctypes.data_as(PD), int(v.shape[0]))
            else:
                M = np.ascontiguousarray(A2, dtype=np.float64)
                rc = sv._lib.ipm_set_A_dense(sv._h, C.c_void_p(M.ctypes.data), M.shape[1], 0)
            assert rc == _lib.IPM_OK
            G.check("after the second A")
            if G.guarded:
                assert _lib.guard_log() == []                   # what the re-setter freed was compared as it was freed
            o = _observe(sv)
            sch = RES._clean(sv)
            assert sch["blocks"] == 2 and sch["fused_small"] == 0
        return o
    _three(monkeypatch, run)


def test_set_then_clear(monkeypatch):
    """The quadratic term, the bounds and both free sets: set, used, cleared, used again; the allocations stay with the handle."""
    free = np.arange(0, 257, 8)
    A, b, c = _lp(130, 257, 52, free=free)
    A0, b0, c0 = _lp(130, 257, 53)
    g, ub = _g(257, 52, every=4), np.where(np.arange(257) % 4 == 1, 3.0, np.inf)

    def run(G):
        o = Obs()
        with G.solver(A, b, c) as sv:                                           # quadratic term + free columns with curvature + bounds
            sv.set_quadratic(g); sv.set_free(free); sv._check(sv._lib.ipm_set_bounds(sv._h, ub.ctypes.data_as(C.POINTER(C.c_double))))
            assert len(sv._sv.guard_bands()) >= 21 + 2 * 3 if G.guarded else True          # quad_g, the marks, bnd_mem
            sv.init_state(1.0)
            o.put("set.iterate3", sv.iterate(3)); o.put("set.state", sv.get_state())
            sv.set_free(None); sv.set_quadratic(None); sv._check(sv._lib.ipm_set_bounds(sv._h, None))
            assert sv.quadratic_nonzeros() == 0 and len(sv.free_columns()) == 0
            sv.set_free_lp(free)                                                # the LP free set on the same handle, then cleared
            sv.init_state(1.0)
            o.put("lp.iterate3", sv.iterate(3)); o.put("lp.state", sv.get_state())
            st = sv.solve(tol=1e-8, max_iter=60)
            o.solves.append((st["status"], st["iterations"])); o.put("lp.solve", st)
            sv.set_free_lp(None)
            assert len(sv.free_lp_columns()[0]) == 0
            RES._clean(sv)
        with G.solver(A0, b0, c0) as sv:                                        # cleared: the plain LP code again, on a plain LP
            sv.set_quadratic(g); sv.set_quadratic(None)
            o = _observe(sv, o, tag="cleared.")
        return o
    _three(monkeypatch, run)


# ---- controls: the instrument sees damage ---------------------------------------------------------------------------------
def _hip():
    """The HIP runtime this process already has loaded (torch's copy), by the path it is mapped from."""
    for line in open("/proc/self/maps"):
        hit = re.search(r"(/\S*libamdhip64\.so\S*)", line)
        if hit:
            lib = C.CDLL(hit.group(1))
            lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            lib.hipDeviceSynchronize.argtypes = []
            return lib
    raise AssertionError("no HIP runtime mapped")


def _poke_workspace(sv, address, value):
    import torch
    sv._ws[address - sv._ws.data_ptr()] = value
    torch.cuda.synchronize()


def _poke_hip(sv, address, value):
    hip = _hip()
    assert hip.hipMemset(C.c_void_p(address), value, 1) == 0 and hip.hipDeviceSynchronize() == 0


def _control(monkeypatch, byte, pick, poke, offsets):
    A, b, c = synthetic_lp(130, 257, seed=11)
    _lib.guard_log()                                            # (what an earlier, failed cell may have left)
    with GB.guard(monkeypatch, byte):
        sv = ipm.IpmSolver(A, b, c, ub=RES._half_bounded(257))
        try:
            sv.init_state(0.0)
            sv.iterate(2)
            GB.assert_intact()
            band = pick(sv)
            planted = []
            for off in offsets(band):
                address, value = band["address"] + off, byte ^ 0x5A
                assert band["address"] <= address < band["address"] + band["bytes"]          # inside memory the library allocated as a band
                poke(sv, address, value)
                bad = sv.guard_check()
                assert [(d["tag"], d["side"], d["address"], d["first_bad"], d["bad_count"]) for d in bad] == \
                    [(band["tag"], band["side"], band["address"], off, 1)], bad
                assert _lib.guard_check() == bad                                            # the process-wide check sees the same
                poke(sv, address, byte)                                                      # restored
                GB.assert_intact()
                planted.append((address, value))
            sv.init_state(0.0)
            st = sv.solve(tol=1e-8, max_iter=60)
            assert st["status"] == 1, st
            GB.assert_intact()
            poke(sv, *planted[0])                                                            # planted again and LEFT: the release must log it
        finally:
            sv.close()
        log = _lib.guard_log()
        assert [(d["tag"], d["side"], d["first_bad"], d["bad_count"]) for d in log] == [(band["tag"], band["side"], planted[0][0] - band["address"], 1)], log
        assert _lib.guard_list() == [] and _lib.guard_log() == []                           # read and cleared


@pytest.mark.parametrize("byte", GB.BYTES)
@pytest.mark.parametrize("where", ["between-nvec-and-mvec", "behind-the-last-region"])
def test_control_workspace(monkeypatch, byte, where):
    tag = "ws:nvec" if where == "between-nvec-and-mvec" else "ws:cval"

    def pick(sv):
        bands = sv.guard_bands()
        assert [d["tag"] for d in bands if d["tag"].startswith("ws:")][-1] == "ws:cval"
        (band,) = [d for d in bands if d["tag"] == tag and d["side"] == 1]
        base = sv._ws.data_ptr()
        assert base <= band["address"] and band["address"] + band["bytes"] <= base + sv.workspace_bytes and band["bytes"] >= GB.BAND
        return band
    _control(monkeypatch, byte, pick, _poke_workspace, lambda band: (0, 4097, band["bytes"] - 1))


@pytest.mark.parametrize("byte", GB.BYTES)
@pytest.mark.parametrize("side", [0, 1])
def test_control_pool_block(monkeypatch, byte, side):
    def pick(sv):
        np_ = (sv.n + 63) // 64 * 64
        cands = [d for d in sv.guard_bands() if not d["tag"].startswith("ws:") and d["inner_bytes"] == 8 * 10 * np_ and d["side"] == side]
        assert len(cands) == 1 and cands[0]["tag"].startswith("ipm_api.hip:") and cands[0]["bytes"] == GB.BAND, cands          # bnd_mem
        return cands[0]
    _control(monkeypatch, byte, pick, _poke_hip, lambda band: (0, band["bytes"] - 1))
