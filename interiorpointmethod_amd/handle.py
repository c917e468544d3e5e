"""IpmSolver: one LP bound to one GPU through a libipm_hip handle.  PyTorch only owns the workspace and the stream; all arithmetic is HIP."""
import collections
import ctypes as C
import os

import numpy as np

from . import _lib
from .analysis import _col, _is_sparse, prepare
# the option checks live in options.py; these names stay importable from here (api.py, batch.py, batches.py, factor_qp.py, the tests)
from .options import (ROUND_OPTIONS, check_correctors, check_detect_qp, check_free, check_free_lp, check_free_rho, check_options, check_quadratic,  # noqa: F401
                      check_refine, check_rounds, check_scale, refuse_correctors, refuse_detect_qp, refuse_free, refuse_free_lp, refuse_quadratic,
                      refuse_refine, refuse_rounds)

STATUS_NAMES = {0: "running", 1: "converged", 2: "max_iter", 3: "nan", 5: "primal_infeasible", 6: "dual_infeasible"}


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def wants_shift(pivots_fixed, m, regularize=0.0, auto_regularize=True):
    """THE 5 % rule of start="mehrotra": with no shift asked for and auto-regularisation allowed, more than 5 % guarded pivots of
    A A^T (dependent rows of A: the QAP family has 9-16 %, every other Netlib file at most 2.7 %) mean the LP is solved with the
    1e-14 Tikhonov shift -- the guard alone stalls the loop there, and a handful of dependent rows is left to the guard
    (the shift breaks 25FV47, BNL1, D6CUBE, WOOD1P, which have 1-11 of them)."""
    return shift_allowed(regularize, auto_regularize) and pivots_fixed > 0.05 * m


def shift_allowed(regularize=0.0, auto_regularize=True):          # may the 5 % rule switch the shift on at all?
    return bool(auto_regularize) and not regularize


def mehrotra_started(make, regularize=0.0, auto_regularize=True):
    """make(**extra) -> IpmSolver.  The solver at Mehrotra's starting point computed on the device (init_state_mehrotra), with the 5 %
    rule applied from the pivot count the start reports: past it, that one handle is recreated with regularize=1e-14 and started
    again.  The caller owns (closes) the solver returned."""
    sv = make()
    try:
        if wants_shift(sv.init_state_mehrotra(), sv.m, regularize, auto_regularize):
            sv.close()
            sv = make(regularize=1e-14)
            sv.init_state_mehrotra()
    except Exception:
        sv.close()
        raise
    return sv


SCALE_PASSES = 16          # default cap of the Ruiz passes: the cap, not a tuning knob


RefineInfo = collections.namedtuple("RefineInfo", "k solves applied half_rule reverts first_rel last_rel max_first_rel")


def _gap_tol(tol, tol_gap):           # the gap tolerance of a solve: tol unless the caller gives one of its own
    return float(tol if tol_gap is None else tol_gap)


class IpmSolver:
    """One LP bound to one GPU: owns a libipm_hip handle whose workspace is a torch tensor."""

    def __init__(self, A, b, c, device=0, eta=0.91, pivot_guard_eps=1e-30, pivot_guard_big=1e64,
                 check_every=4, use_torch=True, dense=False, regularize=0.0, reorder="auto", concurrent=False,
                 auto_regularize=True, factor=None, prepared=None, lockstep=False, ub=None, detect_infeasibility=False,
                 infeasibility_tol=(1e-8, 1e-8), scale=None, scale_passes=SCALE_PASSES, correctors=0, refine=0, dense_cols=None, quad=None,
                 quad_small=False, free=None, lockstep_bounds=False, detect_qp=False, free_lp=None, free_rho=None, free_small=False):
        # (detect_qp, free_lp and free_rho stand IN FRONT of free_small, which an existing test pins as the last parameter: pass them by keyword)
        """check_every: solve() enqueues that many iterations at a time and reads the stop flag once per chunk (the launches behind a
        satisfied stop test return at entry, so the result does not depend on it: DESIGN.md 4-A); a lockstep batch runs chunks of the
        largest value among its members.  IPM_CHECK_EVERY in the environment, when set and not empty, OVERRIDES this argument for
        every solver created while it is set.
        ub: native upper bounds 0 <= x <= ub (length n, +inf = none), checked on the host before any device
        is touched.  The normal matrix keeps order m; a bounded solver joins the lockstep batch only with lockstep_bounds=True.
        lockstep_bounds=True (IPM_FLAG_LOCKSTEP_BOUNDS; off by default, ValueError without lockstep=True): a lockstep solver with a
        finite bound may join solve_lockstep / LockstepBatch, bit-identical to its own solve(), (w, z) included.  The
        flag alone changes nothing (ub None or all +inf: the lockstep solver an unflagged one is) and lifts no other refusal.
        detect_infeasibility: the stop test also tests the iterate for a certificate of primal infeasibility (status 5) or of
        unboundedness (status 6) with the tolerances infeasibility_tol = (eps_p, eps_d) (IPM_FLAG_DETECT_INFEASIBILITY,
        DESIGN.md 4-C); certificate() returns it.  Off by default: the solve is then exactly the reference's loop.
        scale="ruiz": ipm_equilibrate once A, b, c and the bounds are set -- power-of-two Ruiz row / column scaling with at most
        scale_passes passes.  The device then iterates on the scaled LP (stop test, history and statistics are the
        scaled problem's); states, directions and certificates enter and leave in the caller's units, exactly.  scaling() reports
        the factors.  Off by default.
        correctors: up to that many of Gondzio's centrality-corrector rounds per iteration re-use its factorization (set_correctors;
        DESIGN.md 4-G).  0, the default, is the iteration without them, exactly.
        refine: up to that many rounds of iterative refinement behind every normal-equations solve, against the matrix-free
        A D^2 A^T (set_refine).  0, the default, is the iteration without them, exactly.
        dense_cols: None (default: no split), "auto" or a sequence of column indices -- the dense-column split of the sparse factor
        (analysis.prepare, ipm_set_dense_columns).  self.dense_cols is the set in effect (None: none);
        dense_split_info() reports it.  A lockstep solver refuses it (ValueError).
        quad: None (default: the LP) or the diagonal g >= 0 (length n) of a separable convex quadratic term: the solver minimises
        c.x + 1/2 x.diag(g) x (set_quadratic, ipm_set_quadratic), checked on the host before any device is touched.
        The term is set before A, so a small sparse problem takes the multi-kernel path.  lockstep, detect_infeasibility and
        correctors > 0 refuse a nonzero term (ValueError); mehrotra_start / init_state_mehrotra ignore it.
        quad_small=True (IPM_FLAG_SMALL_QUADRATIC; off by default): a problem that qualifies for the fused small path (sparse A, at
        most 128 rows) keeps it with a quadratic term -- the whole loop of the QP in one launch of one workgroup, and the solver may
        join solve_small_batch_solvers; set_quadratic then also accepts a term after construction.  The flag alone changes nothing
        (no term, or a problem that does not qualify: the solver an unflagged one is, bit for bit) and lifts no refusal.
        free: None (default), a sequence of column indices or a boolean mask: the free columns (set_free, ipm_set_free_columns;
        DESIGN.md 4-U) -- columns with quad > 0 and no upper bound that carry no sign constraint, what the factor form of
        Q = diag(g) + F F^T needs (factor_qp.solve_factor_qp builds it).  Checked on the host before any device is touched
        (check_free: ValueError naming the column) and set before A, so a small sparse problem takes the multi-kernel path
        (unless free_small=True, below).
        lockstep, detect_infeasibility and correctors > 0 refuse a non-empty set (ValueError); so does init_state_mehrotra
        (IpmError).  s is 0 on a free column in every state that goes in or comes out.
        free_small=True (IPM_FLAG_SMALL_QUADRATIC | IPM_FLAG_SMALL_FREE; off by default): a problem that qualifies for the fused
        small path keeps it with a quadratic term AND with free columns -- a factor-model QP of m + k <= 128 rows runs its whole
        loop in one launch of one workgroup, the solver may join solve_small_batch_solvers, and set_free is accepted after
        construction too.  Implies what quad_small=True gives.  The flag alone changes nothing and lifts no other refusal.
        detect_qp=True (IPM_FLAG_DETECT_INFEASIBILITY | IPM_FLAG_DETECT_QUADRATIC; off by default): the infeasibility
        tests of a quadratic problem -- with quad (and free) the solve may end in status 5 / 6 with a certificate: a free column
        needs (A^T y)_j = 0, and a ray of unboundedness has -c.x > 0 for the LINEAR objective and avoids the curvature (g o x = 0).
        Implies detect_infeasibility=True (infeasibility_tol applies).  ValueError without a quadratic term and with lockstep=True;
        every other refusal (correctors, init_state_mehrotra with free columns) stays.
        free_lp: None (default), a sequence of column indices or a boolean mask: the LP free columns (set_free_lp,
        ipm_set_free_lp_columns) -- columns of an LP without a sign constraint, served by proximal-point
        regularisation of the free block with the weight free_rho (None or <= 0: the library's default 1e-8; in the units of the
        problem the device iterates on).  Checked on the host before any device is touched (check_free_lp: ValueError naming the
        column) and set before A, so a small sparse problem takes the multi-kernel path.  quad, free, lockstep,
        detect_infeasibility and correctors > 0 refuse a non-empty set (ValueError).  s is 0 on such a column in every state;
        mehrotra_start / init_state_mehrotra serve the set."""
        n_cols = np.asarray(c).reshape(-1).shape[0] if prepared is None else prepared.n
        v = check_options("IpmSolver", n_cols, scale=scale, lockstep=lockstep, lockstep_bounds=lockstep_bounds, correctors=correctors, refine=refine, quad=quad,
                          free=free, detect_qp=detect_qp, free_lp=free_lp, free_rho=free_rho, detect_infeasibility=detect_infeasibility,
                          dense_cols=dense_cols, ub=ub, prepared=prepared)
        self.scale = scale
        correctors, refine, quad, free, detect_qp, free_lp, free_rho = (v[k] for k in ("correctors", "refine", "quad", "free", "detect_qp", "free_lp", "free_rho"))
        if prepared is None:
            prepared = prepare(A, b, c, dense=dense, reorder=reorder, factor=factor, ub=ub, dense_cols=dense_cols)
        self.dense_cols = getattr(prepared, "dense_cols", None)          # (an empty array: the handle's set is cleared explicitly, below)
        self._unsplit_info = getattr(prepared, "unsplit_info", None)
        if lockstep and self.dense_cols is not None and len(self.dense_cols):
            raise ValueError("a lockstep solver has no dense-column split (the Prepared carries dense_cols); solve such LPs one at a time")
        lib = _lib.load()
        self._lib = lib
        self._h = None
        # device row i = caller's row perm[i] (sparse A whose rows the host analysis reordered: minimum degree or RCM)
        self._perm = prepared.perm
        self.m, self.n = prepared.m, prepared.n
        self._host = prepared.host  # the caller's (A, b, c), caller's row order: mehrotra_start and api.unscaled_residuals read it
        self.factor, self.order_info = prepared.factor, prepared.order_info
        A, b, c = prepared.A, prepared.b, prepared.c
        detect_infeasibility = bool(detect_infeasibility) or detect_qp
        opts = _lib.Options()
        lib.ipm_default_options(C.byref(opts))
        opts.eta, opts.pivot_guard_eps, opts.pivot_guard_big = eta, pivot_guard_eps, pivot_guard_big
        opts.check_every = int(os.environ.get("IPM_CHECK_EVERY") or check_every)
        opts.regularize = float(regularize)
        # concurrent=True: this handle shares the GPU with others (batched mode) -- one stream per handle, no look-ahead, no
        # device polling (include/ipm_hip.h: IPM_FLAG_SINGLE_STREAM).  Without it the library still protects itself (it
        # counts the live handles per device and falls back to stream events).
        # lockstep=True: the handle is meant for solve_lockstep (ipm_solve_batch: iteration k of several LPs in the same launches)
        opts.flags = (_lib.FLAG_LOCKSTEP if lockstep else 0) | \
                     ((_lib.FLAG_NO_DEVICE_POLLING | _lib.FLAG_SINGLE_STREAM) if concurrent else 0) | \
                     (0 if auto_regularize else _lib.FLAG_NO_AUTO_REGULARIZE) | \
                     (_lib.FLAG_SPARSE_FACTOR if self.factor == "sparse" else 0) | \
                     (_lib.FLAG_DETECT_INFEASIBILITY if detect_infeasibility else 0) | \
                     (_lib.FLAG_SMALL_QUADRATIC if quad_small or free_small else 0) | \
                     (_lib.FLAG_LOCKSTEP_BOUNDS if lockstep_bounds else 0) | \
                     (_lib.FLAG_SMALL_FREE if free_small else 0) | \
                     (_lib.FLAG_DETECT_QUADRATIC if detect_qp else 0)
        self.quad_small = bool(quad_small)
        self.free_small = bool(free_small)
        self.lockstep_bounds = bool(lockstep_bounds)
        self.detect_infeasibility = bool(detect_infeasibility)
        self.detect_qp = detect_qp
        nbytes = C.c_size_t(0)
        self.sparse = _is_sparse(A)
        if self.sparse:                      # A stays sparse on the device (CSR + CSC, sparse formation of B)
            opts.sparse_nnz = int(A.nnz)
            # (sized from the options: a sparse-factor handle carries no dense m x m normal matrix)
            _lib.check(None, lib.ipm_workspace_bytes_opts(self.m, self.n, C.byref(opts), C.byref(nbytes)))
        else:
            _lib.check(None, lib.ipm_workspace_bytes(self.m, self.n, C.byref(nbytes)))
        self.workspace_bytes = nbytes.value
        ws_ptr, stream = None, None
        self._ws = None
        if use_torch:
            import torch
            if not torch.cuda.is_available():
                raise _lib.IpmLibraryError("no ROCm device visible to torch; the HIP path cannot run")
            dev = torch.device("cuda", device)
            self._ws = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)   # device buffer only
            ws_ptr = C.c_void_p(self._ws.data_ptr())
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        h = C.c_void_p()
        _lib.check(None, lib.ipm_create(int(device), self.m, self.n, C.byref(opts), ws_ptr,
                                        self.workspace_bytes if ws_ptr else 0, stream, C.byref(h)))
        self._h = h
        if quad is not None:                 # before A: ipm_set_A_csc then chooses the one-workgroup small path only with quad_small
            try:
                self._check(lib.ipm_set_quadratic(h, _dptr(quad)))
            except Exception:
                self.close()
                raise
        self._n_free = 0                     # the size of the set the library holds (info["free"] reads it without a library call)
        if free is not None:                 # before A too: a handle with free columns takes the one-workgroup small path only with free_small
            try:
                self._set_free_checked(free)
            except Exception:
                self.close()
                raise
        self._n_free_lp = 0                  # the size of the LP free set the library holds (info["free_lp"])
        self._free_lp_idx = None             # ... and the set itself, for mehrotra_start
        if free_lp is not None:              # before A too: ipm_set_A_csc then takes the multi-kernel path
            try:
                self._set_free_lp_checked(free_lp, free_rho)
            except Exception:
                self.close()
                raise
        if self.sparse:
            indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
            indices = np.ascontiguousarray(A.indices, dtype=np.int32)
            data = np.ascontiguousarray(A.data, dtype=np.float64)
            if self.dense_cols is not None:
                cols = np.ascontiguousarray(self.dense_cols, dtype=np.int32)
                try:
                    self._check(lib.ipm_set_dense_columns(h, int(cols.shape[0]), cols.ctypes.data_as(C.POINTER(C.c_int32))))
                except Exception:
                    self.close()
                    raise
                if not cols.shape[0]:
                    self.dense_cols = None
            self._check(lib.ipm_set_A_csc(h, indptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                          indices.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(data),
                                          int(data.shape[0])))
            if self.factor == "sparse" and self.schedule()["fused_small"]:
                # prepare() never asks for this (analysis._factor_path); a Prepared filled in by other hands may.  The library is the
                # authority: the fused single-workgroup kernel serves the LP, no sparse factor exists: report the path really taken
                self.factor, self.order_info = "dense", None
        else:
            self._check(lib.ipm_set_A_dense(h, C.c_void_p(A.ctypes.data), self.n, 0))
        self.ub = prepared.ub                       # None: no finite bound (the unbounded code runs)
        self.bounded = 0 if self.ub is None else int(np.isfinite(self.ub).sum())
        if self.ub is not None:
            self._check(lib.ipm_set_bounds(h, _dptr(self.ub)))
        self._check(lib.ipm_set_bc(h, _dptr(b), _dptr(c)))
        if detect_infeasibility:
            eps_p, eps_d = infeasibility_tol
            self._check(lib.ipm_set_infeasibility_tol(h, float(eps_p), float(eps_d)))
        self.scale_info = None
        if self.scale is not None:
            info = np.zeros(4)
            ev = None
            if use_torch:          # the handle runs on torch's current stream: two events bracket what ipm_equilibrate enqueues there
                ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev[0].record(torch.cuda.current_stream(dev))
            self._check(lib.ipm_equilibrate(h, int(scale_passes), _dptr(info)))
            ms = None
            if ev is not None:
                ev[1].record(torch.cuda.current_stream(dev))
                ev[1].synchronize()
                ms = float(ev[0].elapsed_time(ev[1]))
            # ms: DEVICE milliseconds of ipm_equilibrate, first launch to last on the handle's stream (the read-back of the pass flags
            # between the passes and the rewrite lies inside; None for a handle without torch, which has no stream to time on)
            self.scale_info = dict(passes=int(info[0]), row_spread_before=float(info[1]), row_spread_after=float(info[2]),
                                   col_spread_after=float(info[3]), ms=ms)
        self.stats = None
        self.correctors = 0
        self.refine = 0
        if self.dense_cols is not None:
            self.refine = self.refine_info().k          # a split handle runs refinement rounds of its own
        try:
            if correctors:
                self.set_correctors(correctors)
            if refine:
                self.set_refine(refine)
        except Exception:
            self.close()
            raise

    # -- plumbing
    def _check(self, code):
        _lib.check(self._h, code)

    def close(self):
        if self._h is not None:
            self._lib.ipm_destroy(self._h)
            self._h = None
            self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state
    def init_state(self, y0=1.0):
        self._check(self._lib.ipm_init_state(self._h, float(y0)))

    def init_state_mehrotra(self):
        """ipm_init_state_mehrotra: Mehrotra's starting point computed on the device from the handle's own A, b, c (and ub) and left
        there as the state -- what set_state(*mehrotra_start()) does with two host round trips, to rounding (the summation orders
        differ).  Returns the guarded pivots of the factorization of A A^T (also last_pivots_fixed): the dependent rows of A."""
        nfix = C.c_int32(0)
        self._check(self._lib.ipm_init_state_mehrotra(self._h, C.byref(nfix)))
        self.last_pivots_fixed = nfix.value
        return nfix.value

    def _rows_in(self, v):          # caller's row order -> device row order
        return v if self._perm is None else np.ascontiguousarray(v[self._perm])

    def _rows_out(self, v):         # device row order -> caller's row order
        if self._perm is None:
            return v
        out = np.empty_like(v)
        out[self._perm] = v
        return out

    def scaling(self):
        """(r, c, info): the power-of-two factors of ipm_equilibrate -- the device solves (R A C, R b, C c, u / C) -- with r in the
        caller's row order, and info = dict(passes, row_spread_before, row_spread_after, col_spread_after) (log2 of max / min over
        the non-empty row / column maxima; None when scale is off).  All ones on an unscaled solver."""
        r, c = np.empty(self.m), np.empty(self.n)
        self._check(self._lib.ipm_get_scaling(self._h, _dptr(r), _dptr(c)))
        return self._rows_out(r), c, self.scale_info

    def set_state(self, x, y, s, w=None, z=None):
        """(w, z): the upper slacks and their duals of a bounded solver (entries outside the bounded set are ignored);
        None keeps what the solver holds (w = z = 1 on the bounded set after construction or init_state)."""
        x, y, s = _col(x, self.n, "x"), self._rows_in(_col(y, self.m, "y")), _col(s, self.n, "s")
        if (w is None) != (z is None):
            raise ValueError("give both w and z or neither")
        if w is not None:
            if not self.bounded:
                raise ValueError("w / z given but the solver has no finite upper bound")
            w, z = _col(w, self.n, "w"), _col(z, self.n, "z")
        self._check(self._lib.ipm_set_state(self._h, _dptr(x), _dptr(y), _dptr(s)))
        if w is not None:
            self._check(self._lib.ipm_set_bound_state(self._h, _dptr(w), _dptr(z)))

    def get_bound_state(self):
        """(w, z) of a bounded solver as (n, 1) arrays (0 outside the bounded set); None without bounds."""
        if not self.bounded:
            return None
        w, z = np.empty(self.n), np.empty(self.n)
        self._check(self._lib.ipm_get_bound_state(self._h, _dptr(w), _dptr(z)))
        return w.reshape(-1, 1), z.reshape(-1, 1)

    def get_state(self):
        x, y, s = np.empty(self.n), np.empty(self.m), np.empty(self.n)
        self._check(self._lib.ipm_get_state(self._h, _dptr(x), _dptr(y), _dptr(s)))
        return x.reshape(-1, 1), self._rows_out(y).reshape(-1, 1), s.reshape(-1, 1)

    # -- seams
    def newton_direction(self, corrector=False):
        dx, dy, ds = np.empty(self.n), np.empty(self.m), np.empty(self.n)
        st = _lib.Stats()
        self._check(self._lib.ipm_newton_direction(self._h, 1 if corrector else 0, _dptr(dx), _dptr(dy),
                                                   _dptr(ds), C.byref(st)))
        self.stats = st.as_dict()
        return dx.reshape(-1, 1), self._rows_out(dy).reshape(-1, 1), ds.reshape(-1, 1)

    def iterate(self, n_steps):
        st = _lib.Stats()
        self._check(self._lib.ipm_iterate(self._h, int(n_steps), C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def solve(self, tol=1e-8, max_iter=5000, tol_gap=None):
        st = _lib.Stats()
        self._check(self._lib.ipm_solve(self._h, float(tol), float(tol), _gap_tol(tol, tol_gap), int(max_iter), C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def history(self):
        """Per-iteration records of the last solve()/iterate() (oldest first; the most recent 1024): list of dicts
        with k, objective, rp_norm, rd_norm, gap, mu, sigma, alpha_aff_p/d, alpha_p/d, pivots_fixed -- the line the
        reference prints per iteration (main.py:808-809, :1186)."""
        buf = (_lib.IterRecord * _lib.HISTORY_CAPACITY)()
        n = C.c_int32(0)
        self._check(self._lib.ipm_get_history(self._h, buf, _lib.HISTORY_CAPACITY, C.byref(n)))
        return [{k: getattr(buf[i], k) for k, _ in _lib.IterRecord._fields_} for i in range(n.value)]

    def _set_rounds(self, name, k):        # the one body of set_correctors / set_refine; self.<name> changes only if the library accepts
        k = check_rounds(name, k)
        self._check(getattr(self._lib, ROUND_OPTIONS[name][1])(self._h, k))
        if name == "refine" and self.dense_cols is not None:
            k = self.refine_info().k          # (a split handle keeps at least its own two rounds)
        setattr(self, name, k)

    def set_quadratic(self, g):
        """ipm_set_quadratic: the diagonal g >= 0 (length n) of the objective's quadratic term from the next iteration on; None or
        all zeros removes it, and the solver runs exactly the LP code again.  Checked on the host first (ValueError: length, NaN,
        Inf, negative); the library refuses a nonzero term (IpmError) on a lockstep solver, with detect_infeasibility, with
        correctors > 0 and, unless the solver was created with quad_small=True, on the fused small path.  Either way the solver
        keeps the term it held."""
        g = check_quadratic(g, self.n)
        self._check(self._lib.ipm_set_quadratic(self._h, None if g is None else _dptr(g)))

    def _set_free_checked(self, idx):
        self._check(self._lib.ipm_set_free_columns(self._h, None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   0 if idx is None else int(idx.shape[0])))
        self._n_free = 0 if idx is None else int(idx.shape[0])

    def set_free(self, free):
        """ipm_set_free_columns: the free columns (indices or a boolean mask) from the next iteration on; None or an empty set
        clears them, and the solver runs exactly the code it ran without.  The indices are checked on the host first (ValueError:
        range, duplicates, every column free); the library decides what depends on the handle's other data (IpmError: a column
        without curvature or with a finite bound, a lockstep or detect_infeasibility solver, the fused small path).  A state the
        solver holds gets s = 0 on the new free columns; after CLEARING, set a state anew (init_state / set_state) before iterating:
        the former free columns still hold s = 0."""
        self._set_free_checked(check_free(free, self.n, term_known=False))

    def free_columns(self):
        """ipm_get_free_columns: the set in the order it was given, as a fresh int32 array (empty: none)."""
        k = C.c_int32(0)
        self._check(self._lib.ipm_get_free_columns(self._h, None, 0, C.byref(k)))
        out = np.zeros(k.value, dtype=np.int32)
        if k.value:
            self._check(self._lib.ipm_get_free_columns(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), k.value, C.byref(k)))
        return out

    def _set_free_lp_checked(self, idx, rho):
        self._check(self._lib.ipm_set_free_lp_columns(self._h, None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      0 if idx is None else int(idx.shape[0]), float(rho)))
        self._n_free_lp = 0 if idx is None else int(idx.shape[0])
        self._free_lp_idx = None if idx is None else idx.copy()

    def set_free_lp(self, free_lp, free_rho=None):
        """ipm_set_free_lp_columns: the LP free columns (indices or a boolean mask) and their proximal weight from the next iteration
        on; None or an empty set clears them, and the solver enqueues exactly what it enqueued without.  The indices and free_rho
        are checked on the host first (ValueError); the library decides what depends on the handle's other data (IpmError: a finite
        bound, a quadratic term, free columns with curvature, a lockstep or detect_infeasibility solver, correctors, the fused small
        path).  A state the solver holds gets s = 0 on the new free columns; after CLEARING, set a state anew before iterating."""
        self._set_free_lp_checked(check_free_lp(free_lp, self.n), check_free_rho(free_rho))

    def free_lp_columns(self):
        """ipm_get_free_lp_columns: (the set in the order it was given as a fresh int32 array, rho in the handle's units)."""
        k, rho = C.c_int32(0), C.c_double(0.0)
        self._check(self._lib.ipm_get_free_lp_columns(self._h, None, 0, C.byref(k), C.byref(rho)))
        out = np.zeros(k.value, dtype=np.int32)
        if k.value:
            self._check(self._lib.ipm_get_free_lp_columns(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), k.value, C.byref(k), C.byref(rho)))
        return out, rho.value

    def debug_column_vector(self, which):
        """ipm_debug_get_column_vector (test hook): "rc", "d", "v" or "q" of the last newton_direction / iterate as the device holds
        it, length n, in the handle's units."""
        out = np.empty(self.n)
        self._check(self._lib.ipm_debug_get_column_vector(self._h, ("rc", "d", "v", "q").index(which), _dptr(out)))
        return out

    def quadratic(self):
        """ipm_get_quadratic: the diagonal in the caller's units as a fresh array of length n (zeros without a term)."""
        g = np.empty(self.n)
        self._check(self._lib.ipm_get_quadratic(self._h, _dptr(g), None))
        return g

    def quadratic_nonzeros(self):
        """The number of positive entries of the term the solver holds (0: the LP)."""
        nz = C.c_int64(0)
        self._check(self._lib.ipm_get_quadratic(self._h, None, C.byref(nz)))
        return int(nz.value)

    def set_correctors(self, k):
        """ipm_set_centrality_correctors: up to k (0 .. MAX_CORRECTORS) centrality-corrector rounds per iteration from the next
        iteration on.  The library refuses k > 0 (IpmError) on a solver on the fused small path and on a lockstep solver; both stay usable."""
        self._set_rounds("correctors", k)

    def corrector_info(self):
        """ipm_get_corrector_info of the last solve() / iterate() sequence: dict with k, rounds (that did work), accepted (rounds)
        and iterations (with at least one accepted round)."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.ipm_get_corrector_info(self._h, out))
        return dict(zip(("k", "rounds", "accepted", "iterations"), (int(v) for v in out)))

    def set_refine(self, k):
        """ipm_set_refinement: up to k (0 .. MAX_REFINE) rounds of iterative refinement behind every normal-equations solve -- the
        iteration's (predictor, corrector, centrality-corrector rounds) and normal_solve's; init_state_mehrotra is not refined.  The
        library refuses k > 0 (IpmError) on a solver on the fused small path and on a lockstep solver; both stay usable."""
        self._set_rounds("refine", k)

    def refine_info(self):
        """ipm_get_refinement_info of the last solve() / iterate() sequence (or normal_solve), in the order of the C array: a
        RefineInfo tuple (k, solves refined, applied corrections, half_rule: rounds ended because the residual did not halve,
        reverts, first_rel / last_rel: the residual norm over ||rhs|| of the most recent solve at its first round and the last one
        kept, max_first_rel)."""
        out = np.zeros(8)
        self._check(self._lib.ipm_get_refinement_info(self._h, _dptr(out)))
        return RefineInfo(*[int(v) for v in out[:5]], *[float(v) for v in out[5:]])

    def debug_refine_vector(self, which):
        """ipm_debug_get_refine_vector (test hook): an m-vector of the last refined solve WITH its padding rows, in the device's row
        order -- which = "t", "r", "delta" (the kept right-hand side, the residual, the correction), "dy" or "dya"."""
        idx = ("t", "r", "delta", "dy", "dya").index(which)
        n = C.c_int64(0)
        self._check(self._lib.ipm_debug_get_refine_vector(self._h, idx, None, 0, C.byref(n)))
        out = np.empty(n.value)
        self._check(self._lib.ipm_debug_get_refine_vector(self._h, idx, _dptr(out), n.value, C.byref(n)))
        return out

    def certificate(self):
        """The certificate of the last solve when it ended in status 5 (primal infeasible) or 6 (dual infeasible, i.e.
        unbounded), else None: dict with kind ("primal_infeasible" / "dual_infeasible"), y (length m, the caller's row order),
        z and x (length n), normalization (beta = b.y - u.z, or gamma = -c.x), violation (of the normalised certificate, as the
        device measured it) and k (iteration of the detection).  Kind 5: A^T y - z <= violation, z >= 0, b.y - u.z = 1 (x = 0);
        kind 6: x >= 0, ||A x||_inf <= violation, c.x = -1 (y = z = 0).  verify_certificate() checks one from the data."""
        if self.stats is None or self.stats["status"] not in (_lib.STATUS_PRIMAL_INFEASIBLE, _lib.STATUS_DUAL_INFEASIBLE):
            return None
        y, z, x, info = np.empty(self.m), np.empty(self.n), np.empty(self.n), np.empty(4)
        self._check(self._lib.ipm_get_certificate(self._h, _dptr(y), _dptr(z), _dptr(x), _dptr(info)))
        return {"kind": STATUS_NAMES[int(info[0])], "y": self._rows_out(y), "z": z, "x": x,
                "normalization": float(info[1]), "violation": float(info[2]), "k": int(info[3])}

    def schedule(self):
        """How the handle runs its factorization (ipm_get_schedule): dict for tests and diagnostics."""
        out = (C.c_int32 * 14)()
        self._check(self._lib.ipm_get_schedule_words(self._h, out, 14, None))
        keys = ("blocks", "group_steps", "grouped_trsv", "device_polling", "counter_steps", "event_steps", "envelope",
                "live_handles", "timeouts_recovered", "fused_small", "fused_factor", "sparse_level_mode", "stream_at", "group_blocks")
        return dict(zip(keys, (int(v) for v in out)))

    def guard_bands(self):
        """The handle's live guard bands (test knob IPM_TEST_ALLOC_GUARD at construction; ipm_debug_guard_list): list of dicts."""
        return _lib.guard_list(self._h)

    def guard_check(self):
        """The damaged ones among them, compared now (ipm_debug_guard_check); [] when every band is intact."""
        return _lib.guard_check(self._h)

    def factor_info(self):
        """Structure of the sparse factor (ipm_get_factor_info) or None for the dense-tile path."""
        if self.factor != "sparse":
            return None
        out = (C.c_int64 * 8)()
        self._check(self._lib.ipm_get_factor_info(self._h, out))
        keys = ("panels", "tasks", "height", "widest_front", "factor_entries", "update_entries", "product_terms",
                "serial_launches")
        return dict(zip(keys, (int(v) for v in out)))

    def dense_split_info(self):
        """ipm_get_dense_split_info: dict with k (dense columns of the split in place), k_padded, row_chunks, factor_entries (of L
        with the split), factor_entries_unsplit (ipm_order_rows' count for the unsplit A where prepare ordered both, else 0),
        factorizations and corrections (since A was set); None for a solver without a split."""
        out = (C.c_int64 * 8)()
        self._check(self._lib.ipm_get_dense_split_info(self._h, out))
        if not out[0]:
            return None
        d = dict(zip(("k", "k_padded", "row_chunks", "factor_entries", "factor_entries_unsplit", "factorizations", "corrections"),
                     (int(v) for v in out)))
        if self._unsplit_info:
            d["factor_entries_unsplit"] = int(self._unsplit_info["nnz_factor"])
        return d

    def debug_dense_split(self, which):
        """ipm_debug_get_dense_split (test hook): "V" or "W" as (m, k) arrays in the DEVICE's row order, "R" (k, k) lower
        triangular, "cols" the column list, "W_stock" W recomputed column by column with the stock forward sweep."""
        idx = ("V", "W", "R", "cols", "W_stock").index(which)
        n = C.c_int64(0)
        self._check(self._lib.ipm_debug_get_dense_split(self._h, idx, None, 0, C.byref(n)))
        out = np.empty(n.value)
        self._check(self._lib.ipm_debug_get_dense_split(self._h, idx, _dptr(out), n.value, C.byref(n)))
        k = len(self.dense_cols)
        if idx < 2 or idx == 4:
            return out.reshape(k, self.m).T.copy()
        return out.reshape(k, k) if idx == 2 else out.astype(np.int64)

    def set_profiling(self, level=2):
        """0 off, 1 time the A D^2 A^T kernel only, 2 all phases (True == 2 for old callers)."""
        level = 2 if level is True else (0 if level is False else int(level))
        self._check(self._lib.ipm_set_profiling(self._h, level))

    def phase_ms(self):
        out = (C.c_double * 4)()
        self._check(self._lib.ipm_get_phase_ms(self._h, out))
        return dict(form=out[0], factor=out[1], trisolve=out[2], other=out[3])

    # -- kernel-level
    def form_normal_matrix(self, d):
        d = _col(d, self.n, "d")
        B = np.empty((self.m, self.m))
        self._check(self._lib.ipm_form_normal_matrix(self._h, _dptr(d), _dptr(B), self.m))
        if self._perm is not None:
            out = np.empty_like(B)
            out[np.ix_(self._perm, self._perm)] = B
            return out
        return B

    def get_factor(self):
        """Lower Cholesky factor of the current normal matrix in DEVICE row order (rows self._perm of the caller's
        A when a reordering was applied)."""
        L = np.empty((self.m, self.m))
        self._check(self._lib.ipm_get_factor(self._h, _dptr(L), self.m))
        return L

    def debug_group_inverse(self, g, which=0):
        """ipm_debug_get_group_inverse (test hook): the explicit inverse of diagonal group g of the current dense factor, whole
        (zero triangle included): which = 0 X_g = inv(L_gg), which = 1 XT_g, its transpose; schedule()["group_blocks"] blocks of
        128 rows each way."""
        rows = 128 * self.schedule()["group_blocks"]
        out = np.empty((rows, rows))
        self._check(self._lib.ipm_debug_get_group_inverse(self._h, int(g), int(which), _dptr(out)))
        return out

    def normal_solve(self, rhs, d=None, reuse_factor=False):
        """z with (A diag(d) A^T) z = rhs on the device (d = None: ones); reuse_factor keeps the previous factor."""
        rhs = self._rows_in(_col(rhs, self.m, "rhs"))
        z = np.empty(self.m)
        dptr = None if d is None else _dptr(_col(d, self.n, "d"))
        nfix = C.c_int32(0)
        self._check(self._lib.ipm_normal_solve(self._h, dptr, _dptr(rhs), _dptr(z), 1 if reuse_factor else 0, C.byref(nfix)))
        self.last_pivots_fixed = nfix.value          # > 0 with d = 1: A A^T is singular, i.e. A has dependent rows
        return self._rows_out(z)

    def mehrotra_start(self):
        """Mehrotra's starting point (SIAM J. Optim. 2 (1992) 575-601, section 7): least-squares x and (y, s), shifted
        into the positive orthant and balanced.  NOT the reference's start (x = s = 1, sparse_interior.py:193-200): an
        optional mode that changes the trajectory; two solves with A A^T on the device, the rest is
        O(nnz) host arithmetic.
        A scaled solver (scale="ruiz") works the recipe on the LP its device holds, (R A C, R b, C c, u / C) -- normal_solve factors
        (R A C)(R A C)^T -- and returns the point unscaled (C x', R y', s' / C, C w', z' / C), which set_state scales back in
        exactly: the start of the scaled LP, as init_state_mehrotra computes it on the device."""
        A, b, c = self._host
        ub, rc = self.ub, None
        if self.scale_info is not None and self.scale_info["passes"]:
            r, cc, _ = self.scaling()
            rc = r, cc
            if _is_sparse(A):
                A = A.copy()          # canonical CSC (analysis.prepare): the values scale in place, the structure stays
                A.data = A.data * r[A.indices] * np.repeat(cc, np.diff(A.indptr))
            else:
                A = r.reshape(-1, 1) * np.asarray(A, dtype=np.float64) * cc.reshape(1, -1)
            b, c = r * np.asarray(b, dtype=np.float64).ravel(), cc * np.asarray(c, dtype=np.float64).ravel()
            ub = None if ub is None else ub / cc
        out = self._mehrotra_start_of(A, np.asarray(b, dtype=np.float64).ravel(), np.asarray(c, dtype=np.float64).ravel(), ub)
        if rc is None:
            return out
        r, cc = rc
        x, y, s = out[0] * cc, out[1] * r, out[2] / cc
        return (x, y, s) if len(out) == 3 else (x, y, s, out[3] * cc, out[4] / cc)

    def _mehrotra_start_of(self, A, b, c, ub):          # the recipe on the LP (A, b, c, ub) that the device holds
        x = A.T @ self.normal_solve(b)
        y = self.normal_solve(A @ c, reuse_factor=True)
        s = c - A.T @ y
        x = np.asarray(x).ravel(); s = np.asarray(s).ravel()
        if self._n_free_lp:
            return self._mehrotra_start_free_lp(x, np.asarray(y).ravel(), s, ub)
        if self.bounded:
            return self._mehrotra_start_bounded(x, np.asarray(y).ravel(), s, ub)
        x = x + max(-1.5 * x.min(), 0.0)
        s = s + max(-1.5 * s.min(), 0.0)
        xs = 0.5 * float(x @ s)
        if not (np.isfinite(xs) and s.sum() > 0 and x.sum() > 0 and xs > 0):
            return np.ones(self.n), np.ones(self.m), np.ones(self.n)          # degenerate data: the reference's start
        x = x + xs / s.sum()
        s = s + xs / x.sum()
        return x, np.asarray(y).ravel(), s

    def _mehrotra_start_bounded(self, x, y, r, ub):
        """Mehrotra's recipe extended to 0 <= x <= u -> (x, y, s, w, z): w = u - x; on U the reduced cost r = c - A^T y splits
        into s = max(r, 0), z = max(-r, 0) (so s - z = r); (x, w) and (s, z) are shifted into the positive orthant together
        and balanced with x.s + w.z.  Outside U, w = z = 0 and s = r as in the unbounded recipe."""
        U = np.isfinite(ub)
        w = np.zeros(self.n); z = np.zeros(self.n)
        w[U] = ub[U] - x[U]
        s = r.copy()
        s[U] = np.maximum(r[U], 0.0)
        z[U] = np.maximum(-r[U], 0.0)
        xmin = min(x.min(), w[U].min())
        smin = min(s.min(), z[U].min())
        dp, dd = max(-1.5 * xmin, 0.0), max(-1.5 * smin, 0.0)
        x = x + dp; w[U] += dp
        s = s + dd; z[U] += dd
        xs = 0.5 * float(x @ s + w[U] @ z[U])
        sx, ss = float(x.sum() + w[U].sum()), float(s.sum() + z[U].sum())
        if not (np.isfinite(xs) and ss > 0 and sx > 0 and xs > 0):
            w[U], z[U] = 1.0, 1.0
            return np.ones(self.n), np.ones(self.m), np.ones(self.n), w, z          # degenerate data: the reference's start
        x = x + xs / ss; w[U] += xs / ss
        sx = float(x.sum() + w[U].sum())                 # (after the primal correction, as in the unbounded recipe)
        s = s + xs / sx; z[U] += xs / sx
        return x, y, s, w, z

    def _mehrotra_start_free_lp(self, x, y, r, ub):
        """The recipe with LP free columns Phi (plain -> (x, y, s), bounded -> (x, y, s, w, z)): on Phi x is the least-squares value,
        unshifted and uncorrected, and s = 0; Phi puts nothing into a minimum or a sum, so the shifts and the balance are those of
        the barrier columns alone -- the arithmetic, in the order of the device start (start_free_lp_* of iteration_rules.h)."""
        F = np.zeros(self.n, dtype=bool)
        F[self._free_lp_idx] = True
        Bc = ~F
        U = np.isfinite(ub) if self.bounded else np.zeros(self.n, dtype=bool)
        w = np.zeros(self.n); z = np.zeros(self.n)
        s = r.copy()
        if self.bounded:
            w[U] = ub[U] - x[U]
            s[U] = np.maximum(r[U], 0.0)
            z[U] = np.maximum(-r[U], 0.0)
        s[F] = 0.0
        x = x.copy()
        dp = max(-1.5 * min(x[Bc].min(), w[U].min() if U.any() else np.inf), 0.0)
        dd = max(-1.5 * min(s[Bc].min(), z[U].min() if U.any() else np.inf), 0.0)
        x[Bc] += dp; w[U] += dp
        s[Bc] += dd; z[U] += dd
        xs = 0.5 * float(x[Bc] @ s[Bc] + w[U] @ z[U])
        sx, ss = float(x[Bc].sum() + w[U].sum()), float(s[Bc].sum() + z[U].sum())
        if not (np.isfinite(xs) and ss > 0 and sx > 0 and xs > 0):          # degenerate data: the reference's start of such a handle
            x, s = np.ones(self.n), np.ones(self.n)
            s[F] = 0.0
            w[U], z[U] = 1.0, 1.0
            return (x, np.ones(self.m), s, w, z) if self.bounded else (x, np.ones(self.m), s)
        x[Bc] += xs / ss; w[U] += xs / ss
        sx = float(x[Bc].sum() + w[U].sum())
        s[Bc] += xs / sx; z[U] += xs / sx
        return (x, y, s, w, z) if self.bounded else (x, y, s)

    def solve_linear(self, B, rhs):
        """B z = rhs for the CALLER's dense SPD matrix (main.py:176-182): the row order this handle keeps its own A in
        plays no part (ipm_solve_linear factors B as given, without the tile envelope or the sparse factor)."""
        B = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
        rhs = _col(rhs, self.m, "rhs")
        z = np.empty(self.m)
        nfix = C.c_int32(0)
        self._check(self._lib.ipm_solve_linear(self._h, _dptr(B), self.m, _dptr(rhs), _dptr(z), C.byref(nfix)))
        return z.reshape(-1, 1), nfix.value
