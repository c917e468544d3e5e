"""The option keywords of the front ends, before any device is touched: the value check of each keyword (check_*), THE table of
which options go together (ROWS) and the one function every front end calls with its keywords (check_options).  DESIGN.md 4-X.

The library holds the same pairs for its handles (csrc/host_compat.h); tests/test_compat_table_host.py compares the two tables."""
import collections

import numpy as np

from . import _lib


def check_scale(scale):
    """THE check of the `scale` keyword, before any device is touched: None (off, the default) or "ruiz"."""
    if scale not in (None, "ruiz"):
        raise ValueError('scale must be None or "ruiz", not %r' % (scale,))
    return scale


# THE table of the round options: keyword -> (its maximum, the library's setter, what the batch front ends lack).  One check, one
# refusal and one setter body (IpmSolver._set_rounds) are built on it.
ROUND_OPTIONS = {
    "correctors": (_lib.MAX_CORRECTORS, "ipm_set_centrality_correctors", "centrality-corrector rounds"),
    "refine": (_lib.MAX_REFINE, "ipm_set_refinement", "refinement rounds"),
}


def check_rounds(name, k):
    """THE check of a round option's keyword, before any device is touched: an integer 0 .. its maximum."""
    kmax = ROUND_OPTIONS[name][0]
    if isinstance(k, bool) or int(k) != k or not 0 <= int(k) <= kmax:
        raise ValueError("%s must be an integer 0 .. %d, not %r" % (name, kmax, k))
    return int(k)


def refuse_rounds(name, k, who):
    """THE refusal of the batch front ends, which have no rounds (lockstep twins, the one-workgroup small kernel): the option is
    checked like anywhere else and k > 0 raises instead of being dropped."""
    if check_rounds(name, k):
        raise ValueError("%s=%d: %s runs no %s; solve such LPs one at a time" % (name, k, who, ROUND_OPTIONS[name][2]))


# the four names their importers use (handle re-exports them; the tests): one-line wrappers
def check_correctors(k): return check_rounds("correctors", k)                 # noqa: E704
def check_refine(k): return check_rounds("refine", k)                         # noqa: E704
def refuse_correctors(k, who): return refuse_rounds("correctors", k, who)     # noqa: E704
def refuse_refine(k, who): return refuse_rounds("refine", k, who)             # noqa: E704


def check_quadratic(quad, n):
    """THE check of the `quad` keyword, before any device is touched: None (no term, the default) or n finite entries >= 0, the
    diagonal g of the objective's quadratic term -> None (also for all zeros: the LP) or a fresh float64 array of length n."""
    if quad is None:
        return None
    g = np.array(quad, dtype=np.float64).reshape(-1)
    if g.shape[0] != n:
        raise ValueError("quad has %d entries, the problem has %d columns" % (g.shape[0], n))
    if not np.all(np.isfinite(g)) or np.any(g < 0):
        raise ValueError("quad must be finite and >= 0 (the diagonal of a convex quadratic term)")
    return g if np.any(g > 0) else None


def _has_term(quad):
    return quad is not None and bool(np.any(np.asarray(quad, dtype=np.float64) > 0))


def refuse_quadratic(quad, who, why):
    """THE refusal of what has no quadratic term: a nonzero term raises instead of being dropped."""
    if _has_term(quad):
        raise ValueError("quad: %s takes no quadratic term (%s)" % (who, why))


def check_index_set(name, cols, n, ub=None):
    """THE check of a keyword that names a set of columns (`free`, `free_lp`): None, a sequence of distinct column indices 0 .. n-1 or
    a boolean mask of length n -> None (also for an empty set) or a fresh int32 array, ascending for a mask and in the caller's order
    otherwise.  A column of such a set carries no bound (ub, None: no bounds, must be +inf there), and one column at least must keep
    its complementarity pair.  Every violation is a ValueError that starts with the keyword and names the column."""
    idx = _index_set(name, cols, n)
    return None if idx is None else _index_set_bounds(name, idx, n, ub)


def _index_set(name, cols, n):           # the first half: the indices themselves -> int64 array or None
    if cols is None:
        return None
    f = np.asarray(cols)
    if f.dtype == np.bool_:
        if f.reshape(-1).shape[0] != n:
            raise ValueError("%s: the mask has %d entries, the problem has %d columns" % (name, f.reshape(-1).shape[0], n))
        idx = np.flatnonzero(f.reshape(-1))
    else:
        f = f.reshape(-1)
        if f.shape[0] and not np.issubdtype(f.dtype, np.integer):
            if not np.issubdtype(f.dtype, np.floating) or not np.all(np.isfinite(f)) or np.any(f != np.floor(f)):
                raise ValueError("%s must be column indices or a boolean mask, not %r" % (name, cols))
        idx = f.astype(np.int64)
    if not idx.shape[0]:
        return None
    seen = set()
    for j in idx.tolist():
        if not 0 <= j < n:
            raise ValueError("%s: column index %d out of range (the problem has %d columns)" % (name, j, n))
        if j in seen:
            raise ValueError("%s: column index %d is given twice" % (name, j))
        seen.add(j)
    return idx


def _index_set_bounds(name, idx, n, ub):           # the second half (check_free puts its curvature rule in between)
    if ub is not None:
        u = np.asarray(ub, dtype=np.float64).reshape(-1)
        if u.shape[0] != n:
            raise ValueError("ub has %d entries, the problem has %d columns" % (u.shape[0], n))
        for j in idx.tolist():
            if np.isfinite(u[j]):
                raise ValueError("%s: column %d has the finite upper bound %r: a free column takes none" % (name, j, float(u[j])))
    if idx.shape[0] >= n:
        raise ValueError("%s: all %d columns free leaves no complementarity pair (mu would be 0/0)" % (name, n))
    return np.ascontiguousarray(idx, dtype=np.int32)


def check_free(free, n, quad=None, ub=None, term_known=True):
    """THE check of the `free` keyword, before any device is touched: an index set (check_index_set) whose columns need curvature --
    with term_known, quad (the diagonal as check_quadratic returns it, None: no term) must be positive there."""
    idx = _index_set("free", free, n)
    if idx is None:
        return None
    if term_known:
        for j in idx.tolist():
            if quad is None or not quad[j] > 0:
                raise ValueError("free: column %d has no quadratic term (quad[%d] = %s): a free column needs curvature, g > 0" % (j, j, "none" if quad is None else repr(float(quad[j]))))
    return _index_set_bounds("free", idx, n, ub)


def _free_count(free):
    """The number of columns a `free` argument names: None 0, a boolean mask its True entries, else its length."""
    if free is None:
        return 0
    f = np.asarray(free)
    return int(f.sum()) if f.dtype == np.bool_ else int(f.size)


def refuse_free(free, who, why):
    """THE refusal of what has no free columns: a non-empty set raises instead of being dropped."""
    if _free_count(free):
        raise ValueError("free: %s takes no free columns (%s)" % (who, why))


def check_free_rho(free_rho):
    """THE check of the `free_rho` keyword: None or a value <= 0 -> 0.0 (the library's default, IPM_FREE_LP_RHO_DEFAULT), a positive
    finite number -> that float; NaN and Inf are a ValueError."""
    if free_rho is None:
        return 0.0
    rho = float(free_rho)
    if not np.isfinite(rho):
        raise ValueError("free_rho = %r is not finite (one positive finite number per solver; None or <= 0: the default %g)" % (free_rho, _lib.FREE_LP_RHO_DEFAULT))
    return rho if rho > 0 else 0.0


def check_free_lp(free_lp, n, ub=None, quad=None, free=None):
    """THE check of the `free_lp` keyword, before any device is touched: an index set (check_index_set).  An LP free column carries
    no quadratic term: the problem must have none (quad) and no free columns with curvature (free) -- the two rows of the table."""
    idx = check_index_set("free_lp", free_lp, n, ub)
    _walk("free_lp pairs", dict(free_lp=idx, quad=quad, free=free))
    return idx


def refuse_free_lp(free_lp, who, why):
    """THE refusal of what has no LP free columns: a non-empty set raises instead of being dropped."""
    if _free_count(free_lp):
        raise ValueError("free_lp: %s takes no LP free columns (%s)" % (who, why))


def check_detect_qp(detect_qp, quad):
    """THE check of the `detect_qp` keyword, before any device is touched: detect_qp=True asks for the infeasibility tests of a
    QUADRATIC problem (IPM_FLAG_DETECT_INFEASIBILITY | IPM_FLAG_DETECT_QUADRATIC) and needs a quadratic term (quad as
    check_quadratic returns it; None: no term) -> bool.  An LP takes detect_infeasibility=True."""
    if detect_qp and quad is None:
        raise ValueError("detect_qp=True without a quadratic term (quad): an LP takes detect_infeasibility=True")
    return bool(detect_qp)


def refuse_detect_qp(detect_qp, who, why):
    """THE refusal of what has no quadratic infeasibility tests (the lockstep front ends): detect_qp=True raises instead of being dropped."""
    if detect_qp:
        raise ValueError("detect_qp: %s takes no quadratic infeasibility tests (%s)" % (who, why))


def refuse_dense_cols(dense_cols, who):
    """THE refusal of the front ends without a split (lockstep twins, the one-workgroup small kernel): the option raises, it is
    never dropped."""
    if dense_cols is not None:
        raise ValueError("dense_cols=%r: %s has no dense-column split; solve such LPs one at a time" % (dense_cols, who))


# ------------------------------------------------------------------------------- which options go together
# A row: keyword `a` is refused beside `b` unless `lifted_by` is on, because `why`.  b is a keyword or, in the rows of a batch front
# end, that front end (it is its own partner: whoever calls it has it on).  `where`: the front ends the row applies to -- SOLVER: IpmSolver
# and solve_with_info; the others by their names.  `text`: the whole message where it is not the refusal of `a` (refuse_<a>) with the
# partner's name and `why`; it may hold one %d, the first column of a.  pair: the library's features of the same row (_lib.FEATURES;
# None: the row lives in the front ends only).  The rows of one front end are walked in table order.
# needs: the row is a requirement -- a is refused where b is OFF.
Row = collections.namedtuple("Row", "where a b lifted_by why text pair needs")
SOLVER, LOCKSTEP_BATCH, SMALL_BATCH, RUN_BATCH = ("IpmSolver", "solve_with_info"), ("the lockstep batch",), ("the small-LP batch",), ("run_batch",)
_ONE_AT_A_TIME = "; solve such problems one at a time"


def _row(where, a, b, why=None, lifted_by=None, text=None, pair=None, needs=False):
    return Row(where, a, b, lifted_by, why, text, pair, needs)


ROWS = (
    # an LP free column carries no quadratic term (check_free_lp walks these two alone: "free_lp pairs")
    _row(SOLVER + ("free_lp pairs",), "free_lp", "quad", pair=("quad", "free_lp"),
         text="free_lp: column %d is an LP free column, but the problem has a quadratic term (quad): a free column with curvature is `free`"),
    _row(SOLVER + ("free_lp pairs",), "free_lp", "free", pair=("free", "free_lp"),
         text="free_lp: column %d is an LP free column, but the problem has free columns with curvature (free): the two sets do not share a solver"),
    _row(("IpmSolver",), "lockstep_bounds", "lockstep", needs=True,
         text="lockstep_bounds=True needs lockstep=True: it opts a lockstep solver into the batch's bounded kernels"),
    _row(SOLVER, "free_lp", "lockstep", "the batch has no free_lp kernels" + _ONE_AT_A_TIME, pair=("free_lp", "lockstep")),
    _row(SOLVER, "free_lp", "detect_infeasibility", "the infeasibility tests are not restated for LP free columns", pair=("free_lp", "detect")),
    _row(SOLVER, "free_lp", "correctors", "the rounds' kernels are not restated for LP free columns", pair=("free_lp", "correctors")),
    _row(SOLVER, "detect_qp", "lockstep", "the batch has no quadratic kernels" + _ONE_AT_A_TIME, pair=("detect_qp", "lockstep")),
    _row(SOLVER, "quad", "lockstep", "the batch has no quadratic kernels" + _ONE_AT_A_TIME, pair=("quad", "lockstep")),
    _row(SOLVER, "quad", "detect_infeasibility", "the infeasibility tests are the LP's", lifted_by="detect_qp", pair=("quad", "detect")),
    _row(SOLVER, "quad", "correctors", "a quadratic solver takes one step length, the rounds compare step pairs", pair=("quad", "correctors")),
    _row(SOLVER, "free", "lockstep", "the batch has no Free kernels" + _ONE_AT_A_TIME, pair=("free", "lockstep")),
    _row(SOLVER, "free", "detect_infeasibility", "the infeasibility tests are the LP's", lifted_by="detect_qp", pair=("free", "detect")),
    _row(SOLVER, "dense_cols", "lockstep", pair=("dense_split", "lockstep")),
    _row(("solve_with_info",), "free", "start", "the least-squares start is not restated for free columns", pair=("mehrotra_start", "free")),
    _row(("IpmSolver",), "ub", "prepared", text="pass ub to prepare() when a Prepared is given"),
    _row(("IpmSolver",), "dense_cols", "prepared", text="pass dense_cols to prepare() when a Prepared is given"),
    # the batch front ends: what their kernels lack
    _row(LOCKSTEP_BATCH, "detect_qp", "the lockstep batch", "the Quad and Free kernels have no batched twins" + _ONE_AT_A_TIME, pair=("detect_qp", "lockstep")),
    _row(LOCKSTEP_BATCH, "free", "the lockstep batch", "the Free kernels have no batched twins" + _ONE_AT_A_TIME, pair=("free", "lockstep")),
    _row(LOCKSTEP_BATCH, "free_lp", "the lockstep batch", "the free_lp kernels have no batched twins" + _ONE_AT_A_TIME, pair=("free_lp", "lockstep")),
    _row(SMALL_BATCH, "free", "the small-LP batch", "the one-workgroup kernel has no free columns" + _ONE_AT_A_TIME),
    _row(SMALL_BATCH, "free_lp", "the small-LP batch", "the one-workgroup kernel has no LP free columns" + _ONE_AT_A_TIME),
    _row(LOCKSTEP_BATCH, "correctors", "the lockstep batch", pair=("correctors", "lockstep")),
    _row(LOCKSTEP_BATCH, "refine", "the lockstep batch", pair=("refinement", "lockstep")),
    _row(LOCKSTEP_BATCH, "dense_cols", "the lockstep batch", pair=("dense_split", "lockstep")),
    _row(SMALL_BATCH, "correctors", "the small-LP batch"),
    _row(SMALL_BATCH, "refine", "the small-LP batch"),
    _row(SMALL_BATCH, "dense_cols", "the small-LP batch"),
    _row(RUN_BATCH, "free", "run_batch", "its problems are LPs" + _ONE_AT_A_TIME),
    _row(RUN_BATCH, "free_lp", "run_batch", "its problems are (A, b, c, ub) tuples with no slot for free columns" + _ONE_AT_A_TIME),
)

# how a keyword's value says "on", and how a partner is named in a message
_ON = {"quad": _has_term, "free": _free_count, "free_lp": _free_count, "start": lambda s: s == "mehrotra", "dense_cols": lambda d: d is not None,
       "ub": lambda u: u is not None, "prepared": lambda p: p is not None}
_NAMED = {"lockstep": "a lockstep solver", "detect_infeasibility": "detect_infeasibility=True", "start": 'start="mehrotra"'}
_REFUSE = {"quad": refuse_quadratic, "free": refuse_free, "free_lp": refuse_free_lp, "detect_qp": refuse_detect_qp}


def _on(kw, name):
    return bool(_ON.get(name, bool)(kw.get(name)))


def _walk(where, kw):
    """Raise the ValueError of the first row of `where`, in table order, whose two sides are on and whose lift is not."""
    for r in ROWS:
        if where not in r.where or not _on(kw, r.a):
            continue
        b_on = r.b in r.where or _on(kw, r.b)              # (a batch front end is its own partner)
        if b_on != (not r.needs) or (r.lifted_by and _on(kw, r.lifted_by)):
            continue
        if r.text:
            raise ValueError(r.text % int(np.asarray(kw[r.a]).reshape(-1)[0]) if "%d" in r.text else r.text)
        who = "correctors=%d" % kw["correctors"] if r.b == "correctors" else _NAMED.get(r.b, r.b)
        if r.a in ROUND_OPTIONS:
            refuse_rounds(r.a, kw[r.a], who)
        elif r.a == "dense_cols":
            refuse_dense_cols(kw[r.a], who)
        else:
            _REFUSE[r.a](kw[r.a], who, r.why)


def check_options(who, n=None, **kw):
    """THE options check of every front end, before any device is touched: `who` (a name of Row.where) passes the keywords it has.
    1. The value checks of the keywords given: scale, correctors, refine and, where the number of columns n is known, quad, free
    (against quad and ub), detect_qp (against quad), free_lp (against ub) and free_rho.  2. The table: the first row of `who` whose two
    sides are on and whose lift is not raises its ValueError.  3. -> the keywords, normalised as their checks return them."""
    v = dict(kw)
    ub = v.get("ub") if v.get("prepared") is None else getattr(v["prepared"], "ub", None)          # (a Prepared carries its bounds)
    if "scale" in v:
        check_scale(v["scale"])
    for name in ("correctors", "refine"):
        if name in v:
            v[name] = check_rounds(name, v[name])
    if n is not None:
        if "quad" in v:
            v["quad"] = check_quadratic(v["quad"], n)
        if "free" in v:
            v["free"] = check_free(v["free"], n, v.get("quad"), ub)
        if "detect_qp" in v:
            v["detect_qp"] = check_detect_qp(v["detect_qp"], v.get("quad"))
        if "free_lp" in v:
            v["free_lp"] = check_index_set("free_lp", v["free_lp"], n, ub)
        if "free_rho" in v:
            v["free_rho"] = check_free_rho(v["free_rho"])
    _walk(who, v)
    return v
