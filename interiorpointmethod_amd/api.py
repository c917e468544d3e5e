"""Host-side mirror of the reference's interior-point call surface, running on libipm_hip.so.

Same names and argument meaning as the reference (payakorn/InteriorPointMethod):

    solve(A, b, c)                      -> (x, y, s)      the north-star seam
    interior_sparse(A, b, c, cTlb, tol) -> objective - cTlb          main.py:760-815
    interior(A, b, c, tol)              -> objective                 main.py:707-757 (returns None there)
    (direction_*, solve_linear: kkt.py)

A is a scipy sparse matrix (any format; the reference passes CSC) or a dense array; b, c are (len,) or (len, 1) of any numeric dtype
(the .mat files hold int16/uint8) and are cast to float64 here.  Outputs are fresh (len, 1) float64 arrays like the reference's."""
import os

import numpy as np

from . import _lib
from .analysis import _upper_bounds
from .handle import SCALE_PASSES, STATUS_NAMES, IpmSolver, mehrotra_started, shift_allowed, wants_shift
from .options import check_free_rho, check_options


def _info(solver, cTlb=0.0):
    st = dict(solver.stats)
    st["status_name"] = STATUS_NAMES.get(st["status"], "?")
    st["rp"] = st["rp_norm"] / (1.0 + st["b_norm"])          # reference scaling, main.py:170
    st["rd"] = st["rd_norm"] / (1.0 + st["c_norm"])          # main.py:171
    st["objective_minus_cTlb"] = st["objective"] - cTlb
    return st


def _solve_info(solver, history=False, certificate=False):
    """THE information record of a solved IpmSolver: _info, the bounded set (with w, z), on request history and certificate, the
    library's hidden recoveries (batch.RECORD_FIELDS): polls that timed out and were rolled back and repeated, sparse-factor sweeps
    that ran as one workgroup after such a time-out (0 where no sparse factor exists), and the factorization path."""
    info = _info(solver)
    info["bounded"] = solver.bounded
    if solver.bounded:
        info["w"], info["z"] = solver.get_bound_state()
    if history:
        info["history"] = solver.history()
    if certificate:
        info["certificate"] = solver.certificate()
    info["timeouts_recovered"] = solver.schedule()["timeouts_recovered"]
    fi = solver.factor_info()
    info["serial_launches"] = fi["serial_launches"] if fi else 0
    info["factor_path"] = solver.factor
    info["correctors"] = solver.corrector_info()
    info["refine"] = solver.refine_info()
    info["dense_cols"] = solver.dense_split_info()          # None: no dense-column split ran
    info["quadratic"] = solver.quadratic_nonzeros()         # positive entries of the quadratic term's diagonal (0: an LP)
    # the path that served a quadratic term: "small" (the one-workgroup loop, quad_small=True), "one-workgroup" (the same loop with free
    # columns, free_small=True: its Free variants) or "multi-kernel"; None for an LP
    small = solver.schedule()["fused_small"]
    info["quadratic_path"] = None if not info["quadratic"] else "multi-kernel" if not small else "one-workgroup" if solver._n_free else "small"
    info["free"] = solver._n_free                           # free columns (0: none); the count the handle keeps, no library call
    info["free_lp"] = solver._n_free_lp                     # LP free columns (0: none), likewise
    if solver.scale is not None:
        info["scale"] = dict(solver.scale_info)
        info["rp_unscaled"], info["rd_unscaled"] = unscaled_residuals(solver)
    return info


def unscaled_residuals(solver):
    """The reference's relative residuals ||A x - b|| / (1 + ||b||) and ||A^T y + s - z - c (- g o x)|| / (1 + ||c||) (main.py:170-171) of the
    iterate the solver RETURNS, against the caller's own data: what the stop test of a scaled solve meant in the caller's units.
    Host arithmetic on the arrays the solver already holds."""
    A, b, c = solver._host
    x, y, s = (np.asarray(v).reshape(-1) for v in solver.get_state())
    b, c = np.asarray(b, dtype=np.float64).reshape(-1), np.asarray(c, dtype=np.float64).reshape(-1)
    rd = np.asarray(A.T @ y).reshape(-1) + s - c
    if solver.bounded:
        rd = rd - solver.get_bound_state()[1].reshape(-1)
    if solver.quadratic_nonzeros():
        rd = rd - solver.quadratic() * x
    rp = np.asarray(A @ x).reshape(-1) - b
    return float(np.linalg.norm(rp) / (1.0 + np.linalg.norm(b))), float(np.linalg.norm(rd) / (1.0 + np.linalg.norm(c)))


_last_info = None


def last_info():
    """Statistics of the most recent solve()/interior*() call in this process."""
    return _last_info


def _auto_regularize():          # the process-wide switch of the 5 % rule (handle.wants_shift)
    return os.environ.get("IPM_AUTO_REGULARIZE", "1") != "0"


def solve_with_info(A, b, c, tol=1e-8, max_iter=5000, y0=1.0, device=0, tol_gap=None, start="reference",
                    history=False, ub=None, detect_infeasibility=False, device_start=False, scale=None, scale_passes=SCALE_PASSES,
                    correctors=0, refine=0, dense_cols=None, quad=None, quad_small=False, free=None, detect_qp=False, free_lp=None, free_rho=None, free_small=False, **opts):
    # (detect_qp, free_lp and free_rho stand IN FRONT of free_small here, in solve and in interior_sparse: an existing test pins free_small as the last
    #  parameter, so it cannot be keyword-only behind it; pass both by keyword)
    """solve() plus the statistics record (iterations, status, objective, rp, rd, gap, ...).
    start="reference": x = s = 1, y = y0 as the reference does; start="mehrotra": IpmSolver.mehrotra_start(), or with
    device_start=True IpmSolver.init_state_mehrotra(): the same start computed on the device (no host copy of A, one
    synchronisation; equal to rounding, so the trajectory may differ in the last bits).
    history=True adds info["history"], the per-iteration records (IpmSolver.history()).  An LP whose A has more
    than 5 % dependent rows (the QAP family) is solved with the 1e-14 Tikhonov shift, switched on by the library
    after the first factorization (info["auto_regularized"] == 1; auto_regularize=False keeps it off).
    ub: native upper bounds 0 <= x <= ub (+inf = none): info["bounded"] = |U| and, when |U| > 0, info["w"], info["z"].
    detect_infeasibility=True: the solve may end in status 5 / 6 (IpmSolver); info["certificate"] = IpmSolver.certificate().
    scale="ruiz": the LP is equilibrated on the device first (IpmSolver); the statistics are then the SCALED problem's, and
    info["scale"], info["rp_unscaled"], info["rd_unscaled"] say what they mean in the caller's units (unscaled_residuals).
    correctors=K: up to K centrality-corrector rounds per iteration (IpmSolver.set_correctors; 0, the default: none);
    info["correctors"] = IpmSolver.corrector_info().  An LP on the fused small path refuses K > 0 (IpmError).
    refine=k: up to k rounds of iterative refinement behind every normal-equations solve (IpmSolver.set_refine; 0, the default:
    none); info["refine"] = IpmSolver.refine_info().  An LP on the fused small path refuses k > 0 (IpmError).
    dense_cols: None (default), "auto" or column indices: the dense-column split of the sparse factor (IpmSolver);
    info["dense_cols"] = IpmSolver.dense_split_info() (None where no split ran).
    quad: None (default) or the diagonal g >= 0 of a separable quadratic term: min c.x + 1/2 x.diag(g) x (IpmSolver; DESIGN.md
    4-Q); info["quadratic"] = its positive entries, info["objective"] includes the term.  Refused (ValueError) together with
    detect_infeasibility and correctors > 0; start="mehrotra" ignores g.
    quad_small=True (off by default): a sparse problem of at most 128 rows keeps the fused small path with its term (IpmSolver,
    IPM_FLAG_SMALL_QUADRATIC); info["quadratic_path"] says which path served the term: "small", "multi-kernel", or None for an LP.
    free: None (default), column indices or a boolean mask: the free columns (IpmSolver) -- quad > 0 there, no bound,
    no sign constraint; info["free"] = their count.  Checked on the host before any device is touched (ValueError naming the
    column); refused (ValueError) together with detect_infeasibility, correctors > 0 and start="mehrotra".
    free_small=True (off by default): a sparse problem of at most 128 rows keeps the fused small path with its term and its free
    columns (IpmSolver, IPM_FLAG_SMALL_FREE); info["quadratic_path"] is then "one-workgroup".
    detect_qp=True (off by default): the infeasibility tests of a QUADRATIC problem (IpmSolver) -- with quad (and
    free) the solve may end in status 5 / 6 and info["certificate"] = IpmSolver.certificate(), which verify_certificate(..., g=quad,
    free=free) checks.  Implies detect_infeasibility=True and lifts its refusal of quad / free; ValueError without a quadratic term.
    free_lp: None (default), column indices or a boolean mask: the LP free columns (IpmSolver) -- free variables of
    an LP, served natively by proximal-point regularisation of the free block with the weight free_rho (None: the library's
    default); info["free_lp"] = their count.  Checked on the host before any device is touched (ValueError naming the column);
    refused (ValueError) together with quad, free, detect_infeasibility and correctors > 0.  Both starts serve the set."""
    global _last_info
    if start not in ("reference", "mehrotra"):
        raise ValueError('start must be "reference" or "mehrotra"')
    n_cols = np.asarray(c).reshape(-1).shape[0]
    ub = _upper_bounds(ub, n_cols)
    v = check_options("solve_with_info", n_cols, scale=scale, correctors=correctors, refine=refine, quad=quad, free=free, detect_qp=detect_qp, free_lp=free_lp,
                      detect_infeasibility=detect_infeasibility, start=start, ub=ub, dense_cols=dense_cols, lockstep=opts.get("lockstep", False))
    correctors, refine, quad, free, detect_qp = (v[k] for k in ("correctors", "refine", "quad", "free", "detect_qp"))
    if scale is not None:
        opts = dict(opts, scale=scale, scale_passes=scale_passes)
    if dense_cols is not None:
        opts = dict(opts, dense_cols=dense_cols)
    if quad_small:
        opts = dict(opts, quad_small=True)
    if free_small:
        opts = dict(opts, free_small=True)
    if detect_qp:
        opts = dict(opts, detect_qp=True)
    if v["free_lp"] is not None:
        check_free_rho(free_rho)                                  # (read only beside a set, as before)
        opts = dict(opts, free_lp=free_lp, free_rho=free_rho)
    detect_infeasibility = bool(detect_infeasibility) or detect_qp
    on_device = start == "mehrotra" and device_start
    if start == "mehrotra" and not on_device and shift_allowed(opts.get("regularize"), _auto_regularize()):
        # the least-squares start factors A A^T: guarded pivots there are dependent rows of A (handle.wants_shift: the 5 % rule).
        # The device start reports the count itself; the host recipe asks a probe handle for it.
        with IpmSolver(A, b, c, device=device, **opts) as probe:
            probe.normal_solve(np.zeros(probe.m))
            if wants_shift(probe.last_pivots_fixed, probe.m):
                opts = dict(opts, regularize=1e-14)
    import time as _time
    t0 = _time.perf_counter()
    if detect_infeasibility:
        opts = dict(opts, detect_infeasibility=True)
    make = lambda **extra: IpmSolver(A, b, c, device=device, ub=ub, correctors=correctors, refine=refine, quad=quad, free=free, **dict(opts, **extra))          # noqa: E731
    with (mehrotra_started(make, opts.get("regularize"), _auto_regularize()) if on_device else make()) as sv:
        t1 = _time.perf_counter()
        if start == "mehrotra" and not on_device:
            sv.set_state(*sv.mehrotra_start())
        elif start == "reference":
            sv.init_state(y0)
        sv.solve(tol=tol, max_iter=max_iter, tol_gap=tol_gap)
        t2 = _time.perf_counter()
        x, y, s = sv.get_state()
        info = _solve_info(sv, history=history, certificate=detect_infeasibility)
    t3 = _time.perf_counter()
    # host-side phases of the call (seconds): handle creation + upload + symbolic analysis, the solve, read-back + destroy
    info["setup_seconds"], info["solve_seconds"], info["teardown_seconds"] = t1 - t0, t2 - t1, t3 - t2
    if os.environ.get("IPM_LP_TIMING"):
        import sys
        print("[lp-timing] m=%d factor=%s setup %.3f solve %.3f (device %.3f) teardown %.3f" %
              (sv.m, info["factor_path"], t1 - t0, t2 - t1, info["solve_ms"] * 1e-3, t3 - t2), file=sys.stderr, flush=True)
    _last_info = info
    return x, y, s, info


def solve(A, b, c, tol=1e-8, max_iter=5000, y0=1.0, device=0, ub=None, scale=None, scale_passes=SCALE_PASSES, correctors=0, refine=0, dense_cols=None,
          quad=None, quad_small=False, free=None, detect_qp=False, free_lp=None, free_rho=None, free_small=False, **opts):
    """min c^T x (+ 1/2 x^T diag(quad) x) s.t. Ax=b, x>=0 (and x <= ub where ub is finite) by the Mehrotra predictor-corrector loop
    on the GPU -> (x, y, s).  quad_small, free (columns without the sign constraint), free_small, detect_qp, free_lp / free_rho (free variables of an LP): as solve_with_info
    (last_info() then holds the status and the certificate of a detection)."""
    x, y, s, _ = solve_with_info(A, b, c, tol=tol, max_iter=max_iter, y0=y0, device=device, ub=ub, scale=scale,
                                 scale_passes=scale_passes, correctors=correctors, refine=refine, dense_cols=dense_cols, quad=quad,
                                 quad_small=quad_small, free=free, detect_qp=detect_qp, free_lp=free_lp, free_rho=free_rho, free_small=free_small, **opts)
    return x, y, s


def _verdict(info, value):
    """+inf for a detected infeasible LP, -inf for a detected unbounded one (the convention of an LP's optimal value)."""
    if info["status"] == _lib.STATUS_PRIMAL_INFEASIBLE:
        return np.inf
    if info["status"] == _lib.STATUS_DUAL_INFEASIBLE:
        return -np.inf
    return value


def interior_sparse(A, b, c, cTlb=0.0, tol=1e-20, device=0, detect_infeasibility=False, scale=None, scale_passes=SCALE_PASSES, correctors=0, refine=0,
                    dense_cols=None, quad=None, free=None, detect_qp=False, free_lp=None, free_rho=None, free_small=False):
    """Drop-in for main.py:760-815: start x=s=y=1, cap 5000, returns sum(x*c) - cTlb (with quad: the quadratic objective - cTlb).  detect_infeasibility=True: +inf for an
    LP detected infeasible, -inf for one detected unbounded.  scale, correctors, refine, dense_cols: as solve_with_info (off by
    default); free likewise (free columns of a quadratic problem), and free_small (the one-workgroup path for them).  detect_qp=True:
    the same verdicts for a problem with quad (solve_with_info): +inf infeasible, -inf unbounded.  free_lp / free_rho: the free
    variables of an LP and their proximal weight, as solve_with_info."""
    _, _, _, info = solve_with_info(A, b, c, tol=tol, max_iter=5000, y0=1.0, device=device,
                                    detect_infeasibility=detect_infeasibility, scale=scale, scale_passes=scale_passes,
                                    correctors=correctors, refine=refine, dense_cols=dense_cols, quad=quad, free=free, detect_qp=detect_qp,
                                    free_lp=free_lp, free_rho=free_rho, free_small=free_small)
    return _verdict(info, info["objective"] - float(cTlb))


def interior(A, b, c, tol=1e-20, device=0, detect_infeasibility=False):
    """Drop-in for main.py:707-757 (dense path: y0=0, cap 50000); returns the objective (detect_infeasibility: as
    interior_sparse)."""
    _, _, _, info = solve_with_info(np.asarray(A, dtype=np.float64), b, c, tol=tol, max_iter=50000, y0=0.0,
                                    device=device, detect_infeasibility=detect_infeasibility)
    return _verdict(info, info["objective"])


def verify_certificate(A, b, c, cert, ub=None, g=None, free=None, F=None):
    """Recompute, in float64 from the problem data alone, how far `cert` (IpmSolver.certificate(): kind, y, z, x; y in the
    caller's row order) is from an exact certificate of min c.x, A x = b, 0 <= x <= ub -> the violation (0 = exact):
      primal_infeasible: y^ = y / t, z^ = z / t with t = b.y - u.z (must be > 0): max(max(A^T y^ - z^)_+, max(-z^)_+);
      dual_infeasible:   x^ = x / t with t = -c.x (must be > 0): max(||A x^||_inf, max(-x^)_+, max x^_U).
    +inf when the normalisation is not positive (no certificate at all).  Pure NumPy / SciPy: no device is touched.
    A quadratic problem min c.x + 1/2 x.(diag(g) + F F^T) x with free columns adds, from the same data alone:
      g (None: no term; the diagonal, length n): max_j g_j |x^_j| joins the dual_infeasible terms (the ray avoids the curvature);
      free (None, column indices or a boolean mask): on a free column max |(A^T y^)_j| replaces the positive part (a free column
        has no slack: equality), and -x^_j is no violation there (no sign constraint);
      F (None, or n x k: the factors of solve_factor_qp's ORIGINAL problem): max |F^T x^| joins the dual_infeasible terms, and a
        primal_infeasible cert may carry y_factor (k), whose |y_factor|_inf joins its terms (the rows F^T x - t = 0 have free t: the
        multipliers must vanish) with F y_factor added to A^T y; a dual_infeasible one may carry t (k), checked as F^T x^ - t^.
    With g, free and F left at None the value is exactly what it was without them."""
    kind = cert["kind"] if isinstance(cert, dict) else cert
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    n = c.shape[0]
    u = np.full(n, np.inf) if ub is None else np.asarray(ub, dtype=np.float64).reshape(-1)
    U = np.isfinite(u)
    phi = np.zeros(n, dtype=bool)
    if free is not None:
        f = np.asarray(free)
        if f.dtype == np.bool_:
            phi = f.reshape(-1).copy()
        else:
            phi[f.astype(np.int64).reshape(-1)] = True
    Fm = None if F is None else np.asarray(F, dtype=np.float64).reshape(n, -1)
    if kind == "primal_infeasible":
        y = np.asarray(cert["y"], dtype=np.float64).reshape(-1)
        z = np.zeros(n) if cert.get("z") is None else np.asarray(cert["z"], dtype=np.float64).reshape(-1)
        z = np.where(U, z, 0.0)
        t = float(b @ y - u[U] @ z[U])
        if not t > 0.0 or not np.isfinite(t):
            return np.inf
        aty = np.asarray(A.T @ y).reshape(-1) / t - z / t
        extra = 0.0
        if Fm is not None and cert.get("y_factor") is not None:
            yf = np.asarray(cert["y_factor"], dtype=np.float64).reshape(-1) / t
            aty = aty + Fm @ yf
            extra = float(np.max(np.abs(yf), initial=0.0))
        if phi.any():
            extra = max(extra, float(np.max(np.abs(aty[phi]), initial=0.0)))
            aty = aty[~phi]
        return float(max(np.max(aty, initial=0.0), np.max(-z / t, initial=0.0), 0.0, extra))
    if kind == "dual_infeasible":
        x = np.asarray(cert["x"], dtype=np.float64).reshape(-1)
        t = float(-(c @ x))
        if not t > 0.0 or not np.isfinite(t):
            return np.inf
        xh = x / t
        ax = np.asarray(A @ xh).reshape(-1)
        v = float(max(np.max(np.abs(ax), initial=0.0), np.max(-xh[~phi] if phi.any() else -xh, initial=0.0), np.max(xh[U], initial=0.0)))
        if g is not None:
            v = max(v, float(np.max(np.asarray(g, dtype=np.float64).reshape(-1) * np.abs(xh), initial=0.0)))
        if Fm is not None:
            ftx = Fm.T @ xh
            v = max(v, float(np.max(np.abs(ftx), initial=0.0)))
            if cert.get("t") is not None:
                v = max(v, float(np.max(np.abs(ftx - np.asarray(cert["t"], dtype=np.float64).reshape(-1) / t), initial=0.0)))
        return v
    raise ValueError("cert kind must be 'primal_infeasible' or 'dual_infeasible', not %r" % (kind,))
