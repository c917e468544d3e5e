"""The batch front ends over IpmSolver handles: the lockstep batch and the small-LP batch (one workgroup per LP)."""
import ctypes as C

import numpy as np

from . import _lib
from .analysis import FUSED_SMALL_MAX_ROWS, _sp, _upper_bounds
from .api import _auto_regularize, _solve_info
from .handle import SCALE_PASSES, IpmSolver, _gap_tol, wants_shift
from .options import check_options, check_quadratic, check_scale


def _handle_array(solvers):           # (the handles as a C array, a Stats array of the same length) for one batched library call
    n = len(solvers)
    return (C.c_void_p * n)(*[sv._h for sv in solvers]), (_lib.Stats * n)()


def _scatter_stats(solvers, stats):           # each solver takes its statistics record (solver.stats) -> the list of them
    for sv, st in zip(solvers, stats):
        sv.stats = st.as_dict()
    return [sv.stats for sv in solvers]


def solve_lockstep(solvers, tol=1e-8, max_iter=5000, tol_gap=None, correctors=0, refine=0, dense_cols=None, free=None, detect_qp=False, free_lp=None):
    """ipm_solve_batch: solve the LPs of `solvers` (IpmSolver objects created with lockstep=True on one device, a state set) AT ONCE,
    iteration k of all of them in the same launches (csrc/lockstep.h) -> list of statistics dicts, one per solver.  Per-LP semantics
    and arithmetic are those of IpmSolver.solve on each of them alone (bit-identical iterates).  Bounded solvers (ub=) join when they
    were created with lockstep_bounds=True, next to unbounded ones, (w, z) bit-identical too; without it the library refuses them
    (IpmError).  correctors > 0: ValueError (the rounds
    have no batched twins; a lockstep solver refuses set_correctors for the same reason); refine > 0 likewise, and free columns, and
    detect_qp=True (no quadratic kernels in the batch)."""
    check_options("the lockstep batch", detect_qp=detect_qp, free=free, free_lp=free_lp, correctors=correctors, refine=refine, dense_cols=dense_cols)          # (ValueError, never dropped)
    hs, st = _handle_array(solvers)
    _lib.check(solvers[0]._h, _lib.load().ipm_solve_batch(hs, len(solvers), tol, tol, _gap_tol(tol, tol_gap), int(max_iter), st))
    return _scatter_stats(solvers, st)


class LockstepBatch:
    """ipm_batch_*: the lockstep batch, incrementally.  add(solver) lets an IpmSolver (lockstep=True, a state set) JOIN between two
    steps; step() runs opt.check_every iterations of every active LP in the same launches and returns the solvers that finished,
    each with its statistics in solver.stats.  A bounded solver joins only with lockstep_bounds=True (IpmError otherwise).  The solvers stay owned by the caller (close them after they are reported finished)."""

    def __init__(self, device=0, tol=1e-8, max_iter=5000, tol_gap=None, stream=None):
        """stream: a torch.cuda.Stream the batch's launches go to (the caller keeps it alive); None: a stream of the batch's own."""
        self._lib = _lib.load()
        self._b = C.c_void_p()
        self._stream = stream
        _lib.check(None, self._lib.ipm_batch_create(int(device), C.c_void_p(stream.cuda_stream) if stream is not None else None, C.byref(self._b)))
        self.tol, self.max_iter, self.tol_gap = float(tol), int(max_iter), _gap_tol(tol, tol_gap)
        self.solvers = []
        self.active = 0

    def _check(self, code):
        if code != _lib.IPM_OK:
            raise _lib.IpmError(code, (self._lib.ipm_batch_last_error(self._b) or b"").decode("utf-8", "replace"))

    def add(self, solver):
        idx = C.c_int32(-1)
        self._check(self._lib.ipm_batch_add(self._b, solver._h, self.tol, self.tol, self.tol_gap, self.max_iter, C.byref(idx)))
        assert idx.value == len(self.solvers)
        self.solvers.append(solver)
        self.active += 1
        return idx.value

    def step(self):
        cap = max(1, len(self.solvers))
        fin = (C.c_int32 * cap)()
        nf, na = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.ipm_batch_step(self._b, fin, cap, C.byref(nf), C.byref(na)))
        self.active = na.value
        out, stats = [self.solvers[fin[k]] for k in range(nf.value)], (_lib.Stats * cap)()
        for k in range(nf.value):
            self._check(self._lib.ipm_batch_stats(self._b, fin[k], C.byref(stats[k])))
        _scatter_stats(out, stats)
        return out

    def schedule(self):
        """ipm_debug_batch_schedule (test hook, host only): the merged schedule the last step() launched -> list of dicts, one per
        launch in order: type (LsType, or LsBndType for a bounded step, of csrc/lockstep.h), members (LPs served by the launch), blocks (the packed grid: the sum of
        the members' own grids) and lds (dynamic LDS bytes).  Empty before the first step."""
        n = C.c_int32(0)
        code = self._lib.ipm_debug_batch_schedule(self._b, None, 0, C.byref(n))
        if n.value == 0:
            self._check(code)
            return []
        out = (C.c_int32 * (4 * n.value))()
        self._check(self._lib.ipm_debug_batch_schedule(self._b, out, 4 * n.value, C.byref(n)))
        return [dict(zip(("type", "members", "blocks", "lds"), (int(v) for v in out[4 * k:4 * k + 4]))) for k in range(n.value)]

    def close(self):
        if self._b:
            self._lib.ipm_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def lockstep_eligible(solver):
    """Can this IpmSolver join solve_lockstep?  Sparse A on the dense-tile factor, more than 128 rows (the small LPs have their fused
    single-workgroup kernel, the sparse-factor LPs their tree sweeps).  A solver with upper bounds only when it was created with
    lockstep_bounds=True (the opt-in to the batch's bounded kernels)."""
    return bool(solver.sparse and solver.factor != "sparse" and (not solver.bounded or solver.lockstep_bounds) and not solver.schedule()["fused_small"])


def small_batch_eligible(solver):
    """Can this IpmSolver join solve_small_batch_solvers?  The library serves it with the fused single-workgroup kernel (sparse A of
    at most 128 rows whose product list fits: ipm_get_schedule out[9] == 1).  Bounds and infeasibility detection do not matter; a
    solver with a quadratic term is on that path, and eligible, only when it was created with quad_small=True, one with free columns
    only with free_small=True."""
    return bool(solver.schedule()["fused_small"])


def solve_small_batch_solvers(solvers, tol=1e-8, max_iter=5000, tol_gap=None, stream=None, correctors=0, refine=0, dense_cols=None):
    """ipm_solve_small_batch: solve the LPs of `solvers` (IpmSolver objects on the fused small-LP path, one device, a state set) in ONE
    launch per kernel variant, one workgroup per LP -> list of statistics dicts, one per solver (also in solver.stats).  Plain,
    bounded and detect_infeasibility solvers may be mixed, and so may solvers that hold a quadratic term on the small path
    (IpmSolver(..., quad=g, quad_small=True), bounded or not: the two Quad variants of the kernel) and solvers with free columns on
    it (free=..., free_small=True: the two Free variants), each of these four also with detect_qp=True (twelve variants in all).  Per-LP semantics and arithmetic are those of IpmSolver.solve on each of
    them alone (bit-identical iterates); get_state / get_bound_state / history / certificate work afterwards as after solve().  The
    solvers stay alive: set_state / init_state and another call re-solve them.  stream: a torch.cuda.Stream for the launches
    (None: the first solver's stream).  ValueError, naming the index, for a solver that is not on the small path, and for
    correctors > 0 or refine > 0 (the one-workgroup kernel runs no centrality-corrector and no refinement rounds)."""
    check_options("the small-LP batch", correctors=correctors, refine=refine, dense_cols=dense_cols)          # (ValueError, never dropped)
    lib = _lib.load()
    solvers = list(solvers)
    if not solvers:
        return []
    for i, sv in enumerate(solvers):
        if not small_batch_eligible(sv):
            raise ValueError("solver %d (%d x %d) is not on the fused small-LP path (sparse A, at most %d rows)"
                             % (i, sv.m, sv.n, FUSED_SMALL_MAX_ROWS))
    hs, st = _handle_array(solvers)
    code = lib.ipm_solve_small_batch(hs, len(solvers), float(tol), float(tol), _gap_tol(tol, tol_gap), int(max_iter),
                                     C.c_void_p(stream.cuda_stream) if stream is not None else None, st)
    _lib.check(None, code)
    return _scatter_stats(solvers, st)


def init_small_batch_mehrotra(solvers, stream=None):
    """ipm_init_small_batch_mehrotra: Mehrotra's starting point (IpmSolver.init_state_mehrotra) for every solver of `solvers` (on the
    fused small-LP path, one device) in ONE launch per kernel variant, one workgroup per LP -> list of the guarded-pivot counts of
    A A^T, one per solver (also in solver.last_pivots_fixed).  Each solver's state is bit-identical to its own init_state_mehrotra().
    stream: a torch.cuda.Stream for the launches (None: the first solver's stream).  ValueError, naming the index, for a solver that
    is not on the small path."""
    lib = _lib.load()
    solvers = list(solvers)
    if not solvers:
        return []
    for i, sv in enumerate(solvers):
        if not small_batch_eligible(sv):
            raise ValueError("solver %d (%d x %d) is not on the fused small-LP path (sparse A, at most %d rows)"
                             % (i, sv.m, sv.n, FUSED_SMALL_MAX_ROWS))
    hs, _ = _handle_array(solvers)
    nfix = (C.c_int32 * len(solvers))()
    _lib.check(None, lib.ipm_init_small_batch_mehrotra(hs, len(solvers), C.c_void_p(stream.cuda_stream) if stream is not None else None, nfix))
    for sv, k in zip(solvers, nfix):
        sv.last_pivots_fixed = int(k)
    return [int(k) for k in nfix]


def _small_batch_host_check(problems, ub):
    """Host part of solve_small_batch (no device is touched): shapes, the row limit of the small path and the bounds ->
    list of (A as CSC, b, c, ub)."""
    if _sp is None:
        raise ImportError("solve_small_batch needs scipy (the small-LP path serves sparse handles)")
    problems = list(problems)
    if ub is not None and len(ub) != len(problems):
        raise ValueError("ub has %d entries, expected one per problem (%d)" % (len(ub), len(problems)))
    out = []
    for i, (A, b, c) in enumerate(problems):
        shape = A.shape if hasattr(A, "shape") else np.asarray(A).shape
        if len(shape) != 2:
            raise ValueError("problem %d: A must be 2-D" % i)
        if shape[0] > FUSED_SMALL_MAX_ROWS:
            raise ValueError("problem %d has %d rows: the small-LP batch serves LPs of at most %d rows"
                             % (i, shape[0], FUSED_SMALL_MAX_ROWS))
        A = _sp.csc_matrix(A, dtype=np.float64)               # dense A too: the small path serves sparse handles
        if A.nnz == 0:
            raise ValueError("problem %d: A has no nonzero entry" % i)
        try:
            u = _upper_bounds(None if ub is None else ub[i], shape[1])
        except ValueError as e:
            raise ValueError("problem %d: %s" % (i, e)) from e
        out.append((A, b, c, u))
    return out


def solve_small_batch(problems, tol=1e-8, max_iter=5000, y0=1.0, device=0, tol_gap=None, ub=None, detect_infeasibility=False,
                      regularize=0.0, start="reference", scale=None, scale_passes=SCALE_PASSES, correctors=0, refine=0, dense_cols=None, free=None, free_lp=None):
    """Solve many small LPs at once -> list of (x, y, s, info), one per problem, each what solve_with_info returns for it alone.

    problems: list of (A, b, c) with at most 128 rows each; a dense A is converted to CSC.  ub: None or one entry per problem (None or
    a length-n vector, +inf = none).  One IpmSolver per LP on the current torch stream, init_state(y0), ONE ipm_solve_small_batch
    call (one workgroup per LP), read-back, close.  start="mehrotra": ONE ipm_init_small_batch_mehrotra call instead of the
    init_state(y0) loop (each LP then equals solve_with_info(start="mehrotra", device_start=True) for it alone; an LP past the 5 % rule
    of handle.wants_shift gets its handle again with regularize=1e-14 and its own start).  An LP the library does not put on the
    small path (more than 128 rows, or a product list of A D^2 A^T beyond its cap) raises ValueError naming its index before anything
    is launched.  scale="ruiz": every LP is equilibrated on the device first (IpmSolver; off by default).  correctors > 0: ValueError
    before any device is touched (solve_small_batch_solvers), and so for refine > 0 and for free columns (free=)."""
    check_options("the small-LP batch", free=free, free_lp=free_lp, correctors=correctors, refine=refine, dense_cols=dense_cols)
    if start not in ("reference", "mehrotra"):
        raise ValueError('start must be "reference" or "mehrotra"')
    check_scale(scale)
    checked = _small_batch_host_check(problems, ub)
    solvers = []
    try:
        for i, (A, b, c, u) in enumerate(checked):
            sv = IpmSolver(A, b, c, device=device, regularize=regularize, ub=u, detect_infeasibility=detect_infeasibility, scale=scale,
                           scale_passes=scale_passes)
            solvers.append(sv)
            if not small_batch_eligible(sv):
                raise ValueError("problem %d (%d x %d) is not served by the fused small-LP path (its product list is too large)"
                                 % (i, sv.m, sv.n))
            if start == "reference":
                sv.init_state(y0)
        if start == "mehrotra":
            for i, nfix in enumerate(init_small_batch_mehrotra(solvers)):
                if wants_shift(nfix, solvers[i].m, regularize, _auto_regularize()):
                    A, b, c, u = checked[i]
                    solvers[i].close()
                    solvers[i] = IpmSolver(A, b, c, device=device, regularize=1e-14, ub=u, detect_infeasibility=detect_infeasibility,
                                           scale=scale, scale_passes=scale_passes)
                    solvers[i].init_state_mehrotra()
        solve_small_batch_solvers(solvers, tol=tol, max_iter=max_iter, tol_gap=tol_gap)
        return [sv.get_state() + (_solve_info(sv, certificate=detect_infeasibility),) for sv in solvers]
    finally:
        for sv in solvers:
            sv.close()


SMALL_TERM_LIMIT = 1 << 22            # ipm_set_A_csc: a product list of more terms leaves the small path (csrc/host_sparse_setup.h)


def _small_qp_batch_host_check(problems, ub):
    """Host part of solve_small_qp_batch (no device is touched): _small_batch_host_check plus the quadratic diagonals ->
    list of (A as CSC, b, c, ub, g or None)."""
    problems = list(problems)
    for i, p in enumerate(problems):
        if len(p) != 4:
            raise ValueError("problem %d: expected (A, b, c, g), got %d entries" % (i, len(p)))
    checked = _small_batch_host_check([(A, b, c) for A, b, c, _ in problems], ub)
    out = []
    for i, ((A, b, c, u), (_, _, _, g)) in enumerate(zip(checked, problems)):
        try:
            g = check_quadratic(g, A.shape[1])
        except ValueError as e:
            raise ValueError("problem %d: %s" % (i, e)) from e
        cnt = np.diff(A.indptr).astype(np.int64)                # a column of c entries feeds c (c + 1) / 2 terms of the product list
        terms = int((cnt * (cnt + 1) // 2).sum())
        if terms > SMALL_TERM_LIMIT:
            raise ValueError("problem %d: the product list of A D^2 A^T has %d terms, the fused small path takes at most %d"
                             % (i, terms, SMALL_TERM_LIMIT))
        out.append((A, b, c, u, g))
    return out


def solve_small_qp_batch_detect(problems, tol=1e-8, max_iter=5000, y0=1.0, device=0, tol_gap=None, ub=None, regularize=0.0, start="reference",
                                scale=None, scale_passes=SCALE_PASSES, infeasibility_tol=(1e-8, 1e-8)):
    """solve_small_qp_batch with the infeasibility tests on every member (the sibling that carries the option: the list of parameters
    of solve_small_qp_batch is fixed): a member with a quadratic term is created with detect_qp=True, an LP in the
    list with detect_infeasibility=True.  An infeasible or unbounded member ends in status 5 / 6 with info["certificate"]
    (IpmSolver.certificate(); None for the others); every other member is, bit for bit, what solve_small_qp_batch returns for it."""
    return _solve_small_qp_batch(problems, tol, max_iter, y0, device, tol_gap, ub, regularize, start, scale, scale_passes, True, infeasibility_tol)


def solve_small_qp_batch(problems, tol=1e-8, max_iter=5000, y0=1.0, device=0, tol_gap=None, ub=None, regularize=0.0, start="reference",
                         scale=None, scale_passes=SCALE_PASSES):
    """Solve many small separable convex QPs at once -> list of (x, y, s, info), one per problem, each what
    solve_with_info(A, b, c, quad=g, quad_small=True) returns for it alone.

    problems: list of (A, b, c, g) with at most 128 rows each: min c.x + 1/2 x.diag(g) x, A x = b, x >= 0 (x <= ub); a dense A is
    converted to CSC.  g: the diagonal, length n, finite and >= 0; None or all zeros is an LP, and LPs may sit in the same list.
    ub, y0, start, regularize, scale: as solve_small_batch (Mehrotra's start ignores g).  Built like solve_small_batch: the host
    check before any device is touched, one IpmSolver(quad=g, quad_small=True) per problem, ONE ipm_solve_small_batch call (one
    workgroup per problem, one grid per kernel variant present), read-back, close.  Every problem error is a ValueError naming the
    problem's index: a bad shape, more than 128 rows, a negative or non-finite g, a product list too large for the path.  The
    front end has no detect_infeasibility (the tests are the LP's), and correctors, refine and dense_cols are not parameters: the
    one-workgroup loop runs none of them, and no free columns either (free is not a parameter, so Python itself
    refuses the keyword).  solve_small_qp_batch_detect is the same call with the infeasibility tests on."""
    return _solve_small_qp_batch(problems, tol, max_iter, y0, device, tol_gap, ub, regularize, start, scale, scale_passes, False, None)


def _solve_small_qp_batch(problems, tol, max_iter, y0, device, tol_gap, ub, regularize, start, scale, scale_passes, detect, infeasibility_tol):
    if start not in ("reference", "mehrotra"):
        raise ValueError('start must be "reference" or "mehrotra"')
    check_scale(scale)
    checked = _small_qp_batch_host_check(problems, ub)

    def make(A, b, c, u, g, reg):
        kw = {}
        if detect:          # (g is None for an LP: check_quadratic)
            kw = dict(infeasibility_tol=infeasibility_tol, **(dict(detect_infeasibility=True) if g is None else dict(detect_qp=True)))
        return IpmSolver(A, b, c, device=device, regularize=reg, ub=u, scale=scale, scale_passes=scale_passes, quad=g, quad_small=True, **kw)
    solvers = []
    try:
        for i, p in enumerate(checked):
            sv = make(*p, regularize)
            solvers.append(sv)
            if not small_batch_eligible(sv):
                raise ValueError("problem %d (%d x %d) is not served by the fused small path (its product list is too large)"
                                 % (i, sv.m, sv.n))
            if start == "reference":
                sv.init_state(y0)
        if start == "mehrotra":
            for i, nfix in enumerate(init_small_batch_mehrotra(solvers)):
                if wants_shift(nfix, solvers[i].m, regularize, _auto_regularize()):
                    solvers[i].close()
                    solvers[i] = make(*checked[i], 1e-14)
                    solvers[i].init_state_mehrotra()
        solve_small_batch_solvers(solvers, tol=tol, max_iter=max_iter, tol_gap=tol_gap)
        return [sv.get_state() + (_solve_info(sv, certificate=detect),) for sv in solvers]
    finally:
        for sv in solvers:
            sv.close()
