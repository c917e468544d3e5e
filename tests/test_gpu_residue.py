"""No result may depend on what device memory held before the library wrote to it.

Every handle runs on memory nobody cleared: the workspace is a torch.empty tensor, everything else comes from a stream-ordered pool
that is kept precisely so that freed blocks are reused.  The rule every kernel has to keep -- write each word before any kernel reads
it, or mask the load -- is invisible to a suite whose allocations are usually zero or finite.  Here each solve path runs three times
on fresh handles: with IPM_TEST_ALLOC_FILL=0, =255 (csrc/host_handle.h: every allocation of the library, the whole workspace
included, is filled with that byte before the library's own first write; as doubles 0xFF is NaN, as integers -1) and with the
variable unset (what production does, on whatever this process left behind).  Every observable is collected as bytes and must be
EQUAL between the three runs, and everything the 255 run returns must be finite.  No tolerance anywhere.

Observables of a cell (_observe): form_normal_matrix(d) with d over 12 decades, both newton_direction results and their scalars,
get_factor(), the state (and bound state) after iterate(3) from init_state, and after solve() the statistics without solve_ms,
history() record by record and pivots_fixed.  Each cell asserts through schedule() / factor_info() that it took the path it names.
Formation by product list against the row-owner kernel (IPM_LIST_FORM) has no schedule word: those two cells rest on the library's
rule (sparse handle, more than 128 rows, at most 1536 padded rows) and on the switch.

THE AUDIT (by reading, before the first filled run): every allocation the knob touches that holds integers, flags or counters; 0xFF
there is -1 / 0xFFFFFFFF, which as an index or an epoch would be a fault or a wait rather than a wrong number.

  buffer                          type          written by (before the first launch that reads it)           first reader
  ------------------------------  ------------  ------------------------------------------------------------  ---------------------------
  tile order (workspace)          int[T]        ipm_create: upload of all T = nblk (nblk + 1) / 2 entries      adat_syrk kernel
  rowptr / colptr (workspace)     int[m+1|n+1]  ipm_set_A_csc: upload of all m + 1 / n + 1 entries             every sparse kernel, rows < m
                                                                                                               and columns < n only
  colind / rowind / rval / cval   int, double   ipm_set_A_csc: upload of the first nz; the tail up to nnz_cap  reached through rowptr /
    (workspace, nnz_cap each)                   is never written and never read (every index is a p with       colptr only
                                                ptr[i] <= p < ptr[i + 1] <= nz; no kernel is given nnz)
  Scalars, history ring, snapshot ints / doubles  ipm_create: memset of [off_inv, off_slab) (set_params_kernel   every kernel (Scalars::done)
    , det, part, fixed (workspace)              then start_solve); `fixed` is in that range and read by nobody
  d_flags (2 nblk + 4)            unsigned      ipm_create: memset 0 of the whole block                        potrf / hand-off kernels,
                                                                                                               time-out + progress words
  d_bulk_done (2 nblk + 4)        unsigned      ipm_create: memset 0 of the whole block                        look-ahead Cholesky
  fused launch: items             FFItem[nit]   ff_build: upload of all nit items                              form_factor_roles_kernel*
  fused launch: tile_items|tile_q int[2 T]      ff_build: two uploads of T entries each                        form_factor_roles_kernel*
  fused launch: flag words        unsigned[2 W] enqueue_form_factor: memset 0 of the W live words before       the launch, ff_gate_kernel
                                                every launch; the second W (diagnostic snapshot) are read by
                                                the host's dumps only (IPM_FF_DEBUG)
  sparse factor: rec, rec_level,  structs, int  build_sparse_factor: sp_upload of the whole host vector; an    sp_form / sp_chol / sp_fwd /
    node, rows, child, crel,                    empty vector gets one unwritten element that no count of the   sp_bwd kernels, eq_spf_apply
    taskptr, tasknode, taskof,                  tables reaches
    fptr, fcol, fcoef, diagpos
  sparse factor: flag (3 nsn),    unsigned,     sp_alloc_zero: memset 0 of the whole block (as L, U, uvec,     sp_chol / sweeps (hand-offs,
    ctr (8)                       unsigned      dinv)                                                          task counter)
  product lists: sm_bptr, sm_bcol int           ipm_set_A_csc: upload of the whole host vector each            small_lp kernels, adat_list,
    , sm_bi / sm_bk, ls_bi / ls_bk                                                                             eq_list_apply
  SmallItem[n] (small batch)      struct        small_batch_round / ipm_init_small_batch_mehrotra: upload of   small_batch_params, the
                                                the cnt entries the launches of that round index (cnt <= n)    small-LP kernels, gather
  Scalars[n] (small batch)        struct        small_batch_gather_kernel writes entries [0, cnt)              the copy to the host, cnt
  LsRec[d_cap] (lockstep)         struct        ipm_batch_step: upload of recs.size() <= d_cap records; every  the lockstep twins
                                                step's (offset, count) lies inside recs
  equilibration scratch           double + int  ipm_equilibrate: memset 0 of the whole block                   eq_* kernels
  bnd_mem (10 np)                 double        ipm_set_bounds: memset 0 of the whole block, then u            bounded kernels
  LU: ipiv[np]                    int           lu_panel_step_kernel: ipiv[k + jj], jj = 0 .. NB - 1, of a     lu_laswp_kernel (panel k),
                                                panel before its lu_laswp_kernel                               the copy to the host
  LU: LuState, bad                struct, int   memset 0 (pval / pidx: each workgroup its slot, then ticket)   lu_panel_step_kernel
  LU: perm[np]                    int           ipm_lu_solve: upload of all np entries                         lu_gather_kernel
No hole was found by reading.

The last cell needs no knob: one handle takes an A, then another A of the same shape with fewer nonzeros and another pattern
(ipm_set_A_csc / ipm_set_A_dense called again through the C entry point), and must return what a fresh handle returns that only
ever saw the second.

Cells dropped: none.  The ragged-groups cell "two-level" forces the grouped Cholesky steps the way test_two_level_blocking_option does
(IPM_GROUP_STEPS).  The file runs in about six seconds on an MI355X.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

import interiorpointmethod_amd as ipm
from interiorpointmethod_amd import _lib
from interiorpointmethod_amd.workloads import synthetic_lp

import infeas_cases as IC
import iteration_oracle as IO
import sparse_cases as SC
import test_gpu_ff_engines as ENG

pytestmark = pytest.mark.gpu

KNOB = "IPM_TEST_ALLOC_FILL"
FILLS = ("0", "255", None)                # None: the variable unset
SP_ENV = ("IPM_SP_MODE", "IPM_SP_GRID", "IPM_SP_FUSE_FWD", "IPM_SP_RELAX", "IPM_FACTOR")


# ---- collecting observables as bytes ---------------------------------------------------------------------------------------
class Obs:
    """name -> bytes, and name -> float array for the finiteness check."""

    def __init__(self):
        self.bytes, self.floats, self.solves = {}, {}, []      # solves: (status, iterations) of every solve() of _observe

    def put(self, key, val):
        if isinstance(val, dict):
            for k in sorted(val):
                if k != "solve_ms":
                    self.put("%s.%s" % (key, k), val[k])
        elif isinstance(val, (list, tuple)):
            self.put(key + ".len", len(val))
            for i, v in enumerate(val):
                self.put("%s[%d]" % (key, i), v)
        elif val is None or isinstance(val, (str, bool, int, np.integer)):
            self.bytes[key] = repr(val).encode()
        else:
            a = np.ascontiguousarray(val)
            self.bytes[key] = a.tobytes()
            if a.dtype.kind == "f":
                self.floats[key] = a


def _three(monkeypatch, run, env=None):
    """run() -> Obs on fresh handles, under fill 0, fill 255 and with the knob unset; the three comparisons."""
    res = {}
    for fill in FILLS:
        with monkeypatch.context() as mp:
            for k, v in (env or {}).items():
                mp.setenv(k, v)
            if fill is None:
                mp.delenv(KNOB, raising=False)
            else:
                mp.setenv(KNOB, fill)
            res[fill] = run()
    zero, ff, unset = (res[f] for f in FILLS)
    assert sorted(zero.bytes) == sorted(ff.bytes) == sorted(unset.bytes)
    differ = [k for k in sorted(zero.bytes) if zero.bytes[k] != ff.bytes[k]]
    assert not differ, ("fill 0 against fill 255", differ)
    nonfinite = [k for k in sorted(ff.floats) if not np.all(np.isfinite(ff.floats[k]))]
    assert not nonfinite, ("fill 255", nonfinite)
    differ = [k for k in sorted(zero.bytes) if unset.bytes[k] != zero.bytes[k]]
    assert not differ, ("knob unset against the filled runs", differ)
    _ran(zero)
    return zero


def _ran(o):
    """Converged or at the cap after at least one iteration: the loop whose results were compared really ran."""
    assert all(status in (1, 2) and k >= 1 for status, k in o.solves), o.solves


def _observe(sv, o=None, max_iter=60, tag=""):
    o = o or Obs()
    d = 10.0 ** np.linspace(-6.0, 6.0, sv.n)                      # 12 decades
    o.put(tag + "B", sv.form_normal_matrix(d))
    sv.init_state(0.0)
    o.put(tag + "affine", sv.newton_direction(False))
    o.put(tag + "affine.stats", sv.stats)
    o.put(tag + "L", sv.get_factor())
    o.put(tag + "corrected", sv.newton_direction(True))
    o.put(tag + "corrected.stats", sv.stats)
    sv.init_state(0.0)
    o.put(tag + "iterate3.stats", sv.iterate(3))
    o.put(tag + "iterate3.state", sv.get_state())
    o.put(tag + "iterate3.bound_state", sv.get_bound_state())
    sv.init_state(0.0)
    st = sv.solve(tol=1e-8, max_iter=max_iter)
    print("OBS solve %d x %d: status %d after %d iterations" % (sv.m, sv.n, st["status"], st["iterations"]))
    o.solves.append((st["status"], st["iterations"]))
    o.put(tag + "solve.stats", st)
    o.put(tag + "solve.pivots_fixed", st["pivots_fixed"])
    o.put(tag + "solve.history", sv.history())
    o.put(tag + "solve.state", sv.get_state())
    o.put(tag + "solve.bound_state", sv.get_bound_state())
    return o


def _clean(sv):
    sch = sv.schedule()
    assert sch["timeouts_recovered"] == 0 and sch["live_handles"] == 1, sch
    return sch


# ---- the LPs ---------------------------------------------------------------------------------------------------------------
def _half_bounded(n):
    """Finite bounds on half the columns, above every x0 of synthetic_lp (U(0.5, 1.5)): the LP stays strictly feasible."""
    return np.where(np.arange(n) % 2 == 0, 3.0, np.inf)


def _feasible(case):
    """The A and u of an iteration_oracle case with a strictly feasible pair (b, c) built from the case's own vectors: b = A min(xb,
    u / 2), c = A^T y + s - z (the cases draw c at random: fine for one iteration, unbounded for a solve)."""
    xf = np.minimum(case.xb, 0.5 * case.u)
    return case.A, case.A @ xf, case.A.T @ case.y + case.s - case.z, case.ub()


# ---- dense ingest, multi-kernel path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,bounded", [(130, 257, False), (130, 257, True), (1, 1, False)], ids=["130x257", "130x257b", "1x1"])
def test_dense_multi_kernel(monkeypatch, m, n, bounded):
    """130 x 257: two blocks, a partial last block, padding rows and columns, a group of 2; with bounds, bnd_mem."""
    A, b, c = synthetic_lp(m, n, seed=11)
    ub = _half_bounded(n) if bounded else None

    def run():
        with ipm.IpmSolver(A, b, c, ub=ub) as sv:
            o = _observe(sv)
            sch = _clean(sv)
            assert not sv.sparse and sv.factor == "dense" and sch["fused_small"] == 0 and sch["fused_factor"] == 0, sch
            assert sch["blocks"] == (m + 127) // 128 and sv.bounded == (0 if ub is None else int(np.isfinite(ub).sum()))
            assert sch["grouped_trsv"] == (1 if m > 128 else 0), sch
        return o
    _three(monkeypatch, run)


RAGGED = {"default": ({}, dict(grouped_trsv=1, group_steps=1)),
          "block-steps": ({"IPM_GROUPED_TRSV": "0"}, dict(grouped_trsv=0, group_steps=1)),
          "two-level": ({"IPM_GROUP_STEPS": "2"}, dict(grouped_trsv=1, group_steps=2))}


@pytest.mark.parametrize("variant", sorted(RAGGED))
def test_ragged_groups(monkeypatch, variant):
    """9 blocks: one group of 8 with explicit inverses (gXT, gX, gS, gPart) and one leftover block solved as a block step."""
    env, want = RAGGED[variant]
    A, b, c = synthetic_lp(1100, 1400, seed=12)

    def run():
        with ipm.IpmSolver(A, b, c) as sv:
            o = _observe(sv)
            sch = _clean(sv)
            assert sch["blocks"] == 9 and sch["fused_factor"] == 0 and sch["fused_small"] == 0, sch
            assert {k: sch[k] for k in want} == want, sch
        return o
    _three(monkeypatch, run, env)


# ---- fused formation + factorization ---------------------------------------------------------------------------------------
FUSED = {"3-blocks": (300, 600, 3, {}), "3-blocks-q1": (300, 600, 3, {"IPM_FF_Q": "1"}), "3-blocks-q16": (300, 600, 3, {"IPM_FF_Q": "16"}),
         "16-blocks-half-pairs": (2048, 4096, 16, {})}


@pytest.mark.parametrize("cell", sorted(FUSED))
def test_fused_formation_and_factorization(monkeypatch, cell):
    """IPM_FUSED_FACTOR=force: 3 blocks with a partial last one, under the default chunking and IPM_FF_Q = 1 and 16 (ff_slab); 16
    blocks, the shape of test_gpu_ff_half_pairs.py (every odd block column has a half-dead tile pair)."""
    m, n, blocks, env = FUSED[cell]
    A, b, c = ENG.problem(m, n)[:3] if m == 2048 else synthetic_lp(m, n, seed=13)

    def run():
        with ipm.IpmSolver(A, b, c) as sv:
            o = _observe(sv)
            sch = _clean(sv)
            assert sch["blocks"] == blocks and sch["fused_factor"] == 1 and sch["device_polling"] == 1, sch
        return o
    _three(monkeypatch, run, dict(env, IPM_FUSED_FACTOR="force"))


# ---- streamed A^T dy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream_at", [1, 0])
def test_streamed_at(monkeypatch, stream_at):
    """2048 x 2500, 16 blocks: the smallest shape of test_gpu_streamed_at.py with a residual stream."""
    A, b, c = synthetic_lp(2048, 2500, seed=7)

    def run():
        with ipm.IpmSolver(A, b, c) as sv:
            o = _observe(sv)
            sch = _clean(sv)
            assert sch["blocks"] == 16 and sch["stream_at"] == stream_at and sch["grouped_trsv"] == 1, sch
        return o
    _three(monkeypatch, run, {} if stream_at else {"IPM_STREAM_AT": "0"})


# ---- the one-workgroup small path and its multi-kernel twin ----------------------------------------------------------------
def _small_lp(name):
    if name == "AFIRO":
        return IC.netlib("AFIRO") + (None,)
    A, b, c, ub = _feasible(IO.get("sparse/" + IO.shape_name(5, 65, True)))
    return sparse.csc_matrix(A), b, c, ub


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["5x65b", "AFIRO"])
def test_small_path(monkeypatch, name, fused):
    A, b, c, ub = _small_lp(name)

    def run():
        with ipm.IpmSolver(A, b, c, ub=ub) as sv:
            o = _observe(sv)
            sch = _clean(sv)
            assert sv.sparse and sv.factor == "dense" and sch["fused_small"] == fused and sch["blocks"] == 1, sch
            assert sv.bounded == (0 if ub is None else int(np.isfinite(ub).sum()))
        return o
    _three(monkeypatch, run, {} if fused else {"IPM_FUSED_SMALL": "0"})


# ---- sparse A, dense factor ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("list_form", [1, 0])
def test_sparse_ingest_dense_factor(monkeypatch, list_form):
    """130 x 257 as CSC, bounded: B from the product list (adat_list_kernel) and, with IPM_LIST_FORM=0, from the row-owner kernel."""
    A, b, c, ub = _feasible(IO.get("sparse/" + IO.shape_name(*IO.SMALL, True)))
    A = sparse.csc_matrix(A)

    def run():
        with ipm.IpmSolver(A, b, c, ub=ub, factor="dense") as sv:
            o = _observe(sv)
            sch = _clean(sv)
            assert sv.sparse and sv.factor == "dense" and sch["fused_small"] == 0 and sch["blocks"] == 2, sch
            assert sv.bounded == int(np.isfinite(ub).sum())
        return o
    _three(monkeypatch, run, {} if list_form else {"IPM_LIST_FORM": "0"})


def _block_bidiagonal():
    """5 row blocks of 100 rows; row block r has entries in column blocks r and r + 1 (150 columns each) only, so rows more than one
    row block apart share no column: with 128-row tiles, tile (3, 0) of A A^T is structurally zero."""
    rng = np.random.default_rng(5)
    R, rows, cols = 5, 100, 150
    blocks = [[None] * (R + 1) for _ in range(R)]
    for r in range(R):
        for k in (r, r + 1):
            M = rng.standard_normal((rows, cols)) * (rng.random((rows, cols)) < 0.08)
            M[np.arange(rows), rng.integers(0, cols, rows)] = 1.0 + rng.random(rows)         # no empty row
            blocks[r][k] = sparse.csc_matrix(M)
    A = sparse.bmat(blocks, format="csc")
    n = A.shape[1]
    x0, y0, s0 = rng.uniform(0.5, 1.5, n), rng.standard_normal(A.shape[0]), rng.uniform(0.5, 1.5, n)
    return A, A @ x0, A.T @ y0 + s0


@pytest.mark.parametrize("envelope", [1, 0])
def test_tiles_outside_the_envelope(monkeypatch, envelope):
    """reorder=None keeps the rows as given: the envelope excludes tile (3, 0), which no formation, panel or update kernel touches
    after the zero fill.  The factor there must be exactly zero under every fill; IPM_ENVELOPE=0 computes it (zeros again)."""
    A, b, c = _block_bidiagonal()
    assert A.shape[0] == 500

    def run():
        with ipm.IpmSolver(A, b, c, factor="dense", reorder=None) as sv:
            assert sv._perm is None
            o = _observe(sv)
            sch = _clean(sv)
            assert sv.sparse and sch["blocks"] == 4 and sch["envelope"] == envelope and sch["fused_small"] == 0, sch
            L = np.frombuffer(o.bytes["L"]).reshape(500, 500)
            assert not np.any(L[384:, :128]) and np.any(L[384:, 256:384])
        return o
    _three(monkeypatch, run, {} if envelope else {"IPM_ENVELOPE": "0"})


# ---- the sparse factor -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["task", "level"])
@pytest.mark.parametrize("name", ["path300", "star106", "bigborder_300_20"])
def test_sparse_factor(monkeypatch, name, mode):
    """A chain 75 panels tall, a wide root, a dense-row supernode (tests/sparse_cases.py), in both walks of the tree; the dense entry
    points on the same handle allocate B_own and invD_own on first use."""
    A, b, c, ub = _feasible(SC.iteration_case(name, False))
    A = sparse.csc_matrix(A)
    rng = np.random.default_rng(3)
    M = rng.standard_normal((A.shape[0], A.shape[0] + 7))
    spd, rhs = M @ M.T + np.eye(A.shape[0]), rng.standard_normal(A.shape[0])
    t = SC.tree(name)

    for k in SP_ENV:
        monkeypatch.delenv(k, raising=False)

    def run():
        with ipm.IpmSolver(A, b, c, ub=ub, factor="sparse") as sv:
            fi = sv.factor_info()
            assert sv.factor == "sparse" and (fi["panels"], fi["height"], fi["widest_front"]) == (t.nsn, t.height, t.rmax), fi
            o = Obs()
            sv.init_state(0.0)
            o.put("first.affine", sv.newton_direction(False))              # before any dense entry point: no B_own yet
            z, nfix = sv.solve_linear(spd, rhs)
            o.put("solve_linear", (z, nfix))
            _observe(sv, o)
            sch = _clean(sv)
            assert sch["sparse_level_mode"] == (1 if mode == "level" else 0) and sv.factor_info()["serial_launches"] == 0, sch
        return o
    _three(monkeypatch, run, {"IPM_SP_MODE": mode})


# ---- batches ---------------------------------------------------------------------------------------------------------------
def test_lockstep_batch_with_a_late_join(monkeypatch):
    """SC205 and E226 (2 blocks), BANDM (3 blocks); BANDM joins between two steps (the record table LsRec is re-merged and grows)."""
    probs = [IC.netlib(nm) for nm in ("SC205", "E226", "BANDM")]

    def run():
        svs = [ipm.IpmSolver(*p, lockstep=True, factor="dense") for p in probs]
        try:
            for sv, blocks in zip(svs, (2, 2, 3)):
                assert ipm.lockstep_eligible(sv) and sv.schedule()["blocks"] == blocks
                sv.init_state(1.0)
            done = []
            with ipm.LockstepBatch(tol=1e-8, max_iter=40) as bt:
                bt.add(svs[0]); bt.add(svs[1])
                done += bt.step()
                bt.add(svs[2])
                for _ in range(60):
                    if not bt.active:
                        break
                    done += bt.step()
                assert bt.active == 0 and sorted(id(s) for s in done) == sorted(id(s) for s in svs)
            o = Obs()
            for i, sv in enumerate(svs):
                o.put("lp%d.stats" % i, sv.stats)
                o.put("lp%d.state" % i, sv.get_state())
                o.put("lp%d.history" % i, sv.history())
                assert sv.schedule()["timeouts_recovered"] == 0
        finally:
            for sv in svs:
                sv.close()
        return o
    _three(monkeypatch, run)


def test_small_batch(monkeypatch):
    """Four LPs of the one-workgroup path in one launch per variant: plain, scaled, bounded and scaled + bounded; Mehrotra's start
    for all of them in one launch (SmallItem, the gathered Scalars), then the batched solve."""
    probs = [IC.netlib(nm) for nm in ("AFIRO", "SC50A", "KB2", "ADLITTLE")]
    opts = [dict(), dict(scale="ruiz"), dict(ub="half"), dict(scale="ruiz", ub="half")]

    def run():
        svs = []
        try:
            for (A, b, c), kw in zip(probs, opts):
                kw = dict(kw)
                if kw.get("ub") == "half":
                    kw["ub"] = np.where(np.arange(A.shape[1]) % 2 == 0, 1e3, np.inf)
                svs.append(ipm.IpmSolver(A, b, c, **kw))
            assert all(sv.schedule()["fused_small"] == 1 for sv in svs)
            o = Obs()
            o.put("start.pivots_fixed", ipm.init_small_batch_mehrotra(svs))
            for i, sv in enumerate(svs):
                o.put("lp%d.start" % i, sv.get_state())
                o.put("lp%d.start.bound_state" % i, sv.get_bound_state())
            stats = ipm.solve_small_batch_solvers(svs, tol=1e-8, max_iter=100)
            for i, (sv, st) in enumerate(zip(svs, stats)):
                o.put("lp%d.stats" % i, st)
                o.put("lp%d.state" % i, sv.get_state())
                o.put("lp%d.bound_state" % i, sv.get_bound_state())
                o.put("lp%d.history" % i, sv.history())
        finally:
            for sv in svs:
                sv.close()
        return o
    _three(monkeypatch, run)


# ---- Mehrotra's start, equilibration, infeasibility certificates -----------------------------------------------------------
@pytest.mark.parametrize("path", ["multi-kernel", "small"])
def test_mehrotra_start_on_a_scaled_handle(monkeypatch, path):
    if path == "small":
        A, b, c = IC.netlib("AFIRO")
    else:
        A, b, c = synthetic_lp(130, 257, seed=14)
        A = A * 2.0 ** np.random.default_rng(1).integers(-12, 13, (130, 1))      # rows over 24 binades: the passes have work to do

    def run():
        with ipm.IpmSolver(A, b, c, scale="ruiz") as sv:
            o = Obs()
            assert sv.scale_info["passes"] >= 1
            o.put("scaling", sv.scaling()[:2])
            o.put("start.pivots_fixed", sv.init_state_mehrotra())
            o.put("start.state", sv.get_state())
            o.put("iterate3.stats", sv.iterate(3))
            o.put("iterate3.state", sv.get_state())
            o.put("history", sv.history())
            sch = _clean(sv)
            assert sch["fused_small"] == (1 if path == "small" else 0) and sch["blocks"] == (1 if path == "small" else 2), sch
        return o
    _three(monkeypatch, run)


@pytest.mark.parametrize("name", ["primal_dense", "dual_dense"])
def test_infeasibility_certificate(monkeypatch, name):
    """cert_mem is allocated by the first certificate() and never cleared."""
    P = IC.small_instances()[name]()

    def run():
        with ipm.IpmSolver(P["A"], P["b"], P["c"], detect_infeasibility=True) as sv:
            sv.init_state(1.0)
            st = sv.solve(tol=1e-8, max_iter=200)
            assert st["status"] == IC.KIND[P["kind"]], st
            o = Obs()
            o.put("stats", st)
            o.put("certificate", sv.certificate())
            o.put("history", sv.history())
            o.put("state", sv.get_state())
            _clean(sv)
        return o
    _three(monkeypatch, run)


# ---- device LU -------------------------------------------------------------------------------------------------------------
def test_device_lu(monkeypatch):
    """130 x 130, 9 right-hand sides (two substitution groups), every leading dimension larger than its row."""
    n, k, lda, ldb, ldx = 130, 9, 137, 12, 11
    rng = np.random.default_rng(130)
    A = np.zeros((n, lda)); A[:, :n] = rng.standard_normal((n, n)); A[np.arange(n), rng.permutation(n)] += 2.0 * np.sqrt(n)
    B = np.zeros((n, ldb)); B[:, :k] = rng.standard_normal((n, k))
    PD, lib = C.POINTER(C.c_double), _lib.load()

    def run():
        X, LU, piv, info = np.zeros((n, ldx)), np.zeros((n, lda)), np.zeros(n, dtype=np.int32), C.c_int64(-1)
        rc = lib.ipm_lu_solve(0, n, A.ctypes.data_as(PD), lda, k, B.ctypes.data_as(PD), ldb, X.ctypes.data_as(PD), ldx, C.byref(info))
        assert rc == _lib.IPM_OK and info.value == 0, (rc, info.value)
        rc = lib.ipm_lu_factor(0, n, A.ctypes.data_as(PD), lda, LU.ctypes.data_as(PD), lda, piv.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info))
        assert rc == _lib.IPM_OK and info.value == 0, (rc, info.value)
        o = Obs()
        o.put("X", X[:, :k]); o.put("LU", LU[:, :n]); o.put("piv", piv)
        assert not np.any(X[:, k:]) and not np.any(LU[:, n:])                     # the pitch is skipped, not written
        return o
    o = _three(monkeypatch, run)
    X = np.frombuffer(o.bytes["X"]).reshape(n, k)
    assert np.linalg.norm(A[:, :n] @ X - B[:, :k]) <= 1e-10 * np.linalg.norm(B[:, :k])


# ---- real residue: a handle that takes a second A --------------------------------------------------------------------------
def _second_A(kind):
    A1, b, c, ub = _feasible(IO.get("sparse/" + IO.shape_name(*IO.SMALL, True)))
    rng = np.random.default_rng(77)
    A2 = np.roll(A1, 3, axis=1) * (rng.random(A1.shape) < 0.6)                     # another pattern, fewer nonzeros
    A2[np.arange(A2.shape[0]), rng.integers(0, A2.shape[1], A2.shape[0])] = 1.5     # no empty row
    assert np.count_nonzero(A2) < np.count_nonzero(A1)
    x0 = rng.uniform(0.5, 1.0, A2.shape[1])
    b2, c2 = A2 @ np.minimum(x0, 0.5 * ub), A2.T @ rng.standard_normal(A2.shape[0]) + rng.uniform(0.5, 1.5, A2.shape[1])
    if kind == "sparse":
        return sparse.csc_matrix(A1), sparse.csc_matrix(A2), b2, c2, ub
    return A1, A2, b2, c2, ub


# ipm_newton_direction reports the handle's whole scalar record (fill_stats); what a direction seam does not compute itself is what
# the library's own last iteration wrote there -- the handle's state, not residue: zero on a fresh handle, the first LP's last
# step on the re-used one.  Everything else, the scalars the seams do compute included, is compared.
CARRIED = {"%s.stats.%s" % (seam, f) for seam, fields in (("affine", ("iterations", "alpha_p", "alpha_d", "mu_aff", "sigma", "objective_last_finite")),
                                                          ("corrected", ("iterations", "alpha_p", "alpha_d", "objective_last_finite")))
           for f in fields}


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_a_reused_handle_equals_a_fresh_one(kind):
    """No knob: what the first A left in the CSR / CSC arrays beyond the second one's nonzeros, in the product lists and in the dense
    image must not reach any result."""
    A1, A2, b, c, ub = _second_A(kind)
    kw = dict(factor="dense", reorder=None) if kind == "sparse" else {}
    with ipm.IpmSolver(A2, b, c, ub=ub, **kw) as sv:
        fresh = _observe(sv)
    with ipm.IpmSolver(A1, b, c, ub=ub, **kw) as sv:
        assert sv._perm is None and sv.sparse == (kind == "sparse")
        _observe(sv, max_iter=5)                                                    # the first A is really used
        PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        if kind == "sparse":
            ip, ix, v = A2.indptr.astype(np.int32), A2.indices.astype(np.int32), A2.data.astype(np.float64)
            rc = sv._lib.ipm_set_A_csc(sv._h, ip.ctypes.data_as(PI), ix.ctypes.data_as(PI), v.ctypes.data_as(PD), int(v.shape[0]))
        else:
            M = np.ascontiguousarray(A2, dtype=np.float64)
            rc = sv._lib.ipm_set_A_dense(sv._h, C.c_void_p(M.ctypes.data), M.shape[1], 0)
        assert rc == _lib.IPM_OK
        reused = _observe(sv)
        sch = _clean(sv)
        assert sch["blocks"] == 2 and sch["fused_small"] == 0
    assert sorted(fresh.bytes) == sorted(reused.bytes)
    differ = [k for k in sorted(fresh.bytes) if fresh.bytes[k] != reused.bytes[k] and k not in CARRIED]
    assert not differ, " ".join(differ)
    assert all(np.all(np.isfinite(a)) for a in reused.floats.values())
    _ran(reused)
